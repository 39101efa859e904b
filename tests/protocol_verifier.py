"""A plain verifier of the protocols the library proves -- sum-checks of  sum_b eq(z, b) g(b)  and of  sum_b g(b), the layered
descents of a product tree and of a fraction tree -- on model elements only: the caller supplies zero, one, add, sub and mul (and the
base prime, for the scalar inverses of the interpolation), as tools/model_*.py and Model of tests/test_mle_gpu.py take them, so the
same code runs on integers modulo a prime, on toy rings whose product is not slot-wise, on the power-of-two rings slot by slot and
on memory images of the reference's own rings with the oracle's Fq3 / Fq9 / Fq4 slot products.

Nothing here is taken from a model of the prover: no fold, no per-pair weights, no factored range polynomial, no offsets into a
buffer of layers.  Every quantity is its definition: a multilinear extension is the sum over the cube of its Lagrange basis, eq is
the product of its n factors, a round polynomial is interpolated through all of its points, a range polynomial multiplies all
2 B - 1 factors.  Variable 0 is the lowest bit of a table index.

A helper module: no test is collected from it (tests/test_protocol_verifier_host.py shows that it can reject, tests/test_protocols_gpu.py
runs the device provers against it).
"""
import numpy as np

LEADING, TRAILING = 0, 1   # which variable a round binds first: variable 0 (leading) or variable n - 1 (trailing)
# the reasons of a rejection
SUM, LENGTH, FINAL, EQ, CLAIM, POINT, ROOT, LEAVES = "sum", "length", "final", "eq", "claim", "point", "root", "leaves"


class Rejected(Exception):
    """round: the round (1 ..) whose check failed, or None where the failure is behind the rounds; reason: one of the names above;
    layer: the layer of a tree whose claim was being checked, or None"""

    def __init__(self, round, reason, layer=None, detail=""):
        super().__init__("layer %s round %s: %s %s" % (layer, round, reason, detail))
        self.round, self.reason, self.layer = round, reason, layer


def same(a, b):
    """equality of two model elements: integers, tuples, or numpy arrays of canonical values"""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


class Verifier:
    def __init__(self, zero, one, add, sub, mul, p):
        """p: the prime of the base field, whose elements R::from embeds"""
        self.zero, self.one, self.add, self.sub, self.mul, self.p = zero, one, add, sub, mul, p

    # ---- the base field in the ring -------------------------------------------------------------------------------------------------
    def scalar(self, c):
        """R::from(c) for an integer c (taken modulo p), from one() by double-and-add"""
        c %= self.p
        out, power = self.zero, self.one
        while c:
            if c & 1:
                out = self.add(out, power)
            power = self.add(power, power)
            c >>= 1
        return out

    def inv_scalar(self, c, p=None):
        p = self.p if p is None else p
        return self.scalar(pow(c % p, -1, p))

    def sum(self, elems):
        total = self.zero
        for e in elems:
            total = self.add(total, e)
        return total

    def prod(self, elems):
        total = self.one
        for e in elems:
            total = self.mul(total, e)
        return total

    # ---- multilinear extensions -----------------------------------------------------------------------------------------------------
    def eq_eval(self, z, r):
        """prod_i (z_i r_i + (1 - z_i)(1 - r_i))"""
        assert len(z) == len(r)
        one, add, sub, mul = self.one, self.add, self.sub, self.mul
        return self.prod(add(mul(zi, ri), mul(sub(one, zi), sub(one, ri))) for zi, ri in zip(z, r))

    def basis(self, point, b):
        """prod_i (b_i ? x_i : 1 - x_i), b_i bit i of the index b"""
        return self.prod(x if (b >> i) & 1 else self.sub(self.one, x) for i, x in enumerate(point))

    def mle_eval(self, table, point, pad=None):
        """sum_b basis(point, b) table[b] over all 2^len(point) indices; the entries that are not stored are `pad` (default zero)"""
        pad = self.zero if pad is None else pad
        assert len(table) <= 1 << len(point)
        return self.sum(self.mul(self.basis(point, b), table[b] if b < len(table) else pad) for b in range(1 << len(point)))

    def bits(self, b, n):
        """the index b as a point of the cube"""
        return [self.one if (b >> i) & 1 else self.zero for i in range(n)]

    # ---- round polynomials ----------------------------------------------------------------------------------------------------------
    def interpolate(self, msg, r):
        """the polynomial of degree < len(msg) through (j, msg[j]) at the ring element r:
        sum_i msg[i] prod_{j != i} (r - R::from(j)) / (i - j); only base-field scalars are inverted"""
        n = len(msg)
        factors = [self.sub(r, self.scalar(j)) for j in range(n)]
        total = self.zero
        for i in range(n):
            den = 1
            for j in range(n):
                if j != i:
                    den = den * (i - j) % self.p
            num = self.prod(f for j, f in enumerate(factors) if j != i)
            total = self.add(total, self.mul(self.mul(num, self.inv_scalar(den)), msg[i]))
        return total

    def verify_rounds(self, claim, messages, challenges, points=None, layer=None):
        """per round: msg[0] + msg[1] == claim, then claim = msg's polynomial at the round's challenge.  points: the number of elements
        a message must have (the degree bound), where the caller knows it.  Returns the last claim."""
        assert len(messages) == len(challenges)
        for j, (msg, r) in enumerate(zip(messages, challenges), start=1):
            if len(msg) < 2 or (points is not None and len(msg) != points):
                raise Rejected(j, LENGTH, layer)
            if not same(self.add(msg[0], msg[1]), claim):
                raise Rejected(j, SUM, layer)
            claim = self.interpolate(msg, r)
        return claim

    @staticmethod
    def point_of(challenges, order):
        """the challenges as a point in variable order: round j bound variable j - 1 (leading) or n - j (trailing)"""
        return list(challenges) if order == LEADING else list(reversed(challenges))

    # ---- whole sum-checks -----------------------------------------------------------------------------------------------------------
    def verify_sumcheck(self, claim0, messages, challenges, finals, order, g_of, tables, pad=None, points=None):
        """sum_b g(b) = claim0 with g a polynomial g_of of the tables' values: the rounds; every final value is the table's extension at
        the point, from the raw table; the last claim is g_of(finals)"""
        last = self.verify_rounds(claim0, messages, challenges, points)
        point = self.point_of(challenges, order)
        if len(finals) != len(tables):
            raise Rejected(None, FINAL)
        for i, (f, t) in enumerate(zip(finals, tables)):
            if not same(f, self.mle_eval(t, point, pad)):
                raise Rejected(None, FINAL, detail="table %d" % i)
        if not same(last, g_of(finals)):
            raise Rejected(None, CLAIM)
        return point

    def verify_eq_sumcheck(self, claim0, z, messages, challenges, finals, eq_r, order, g_of, tables, pad=None, points=None):
        """sum_b eq(z, b) g(b) = claim0: the rounds; every final value from the raw table; eq_r = eq(z, point); the last claim is
        eq_r g_of(finals).  Returns the point."""
        last = self.verify_rounds(claim0, messages, challenges, points)
        point = self.point_of(challenges, order)
        if len(finals) != len(tables):
            raise Rejected(None, FINAL)
        for i, (f, t) in enumerate(zip(finals, tables)):
            if not same(f, self.mle_eval(t, point, pad)):
                raise Rejected(None, FINAL, detail="table %d" % i)
        if not same(eq_r, self.eq_eval(z, point)):
            raise Rejected(None, EQ)
        if not same(last, self.mul(eq_r, g_of(finals))):
            raise Rejected(None, CLAIM)
        return point

    def _layer(self, claim0, z, t, g_of, points, layer):
        """the sum-check of one layer of a tree, in trailing order.  The verifier holds no table of the layer below: the final values
        are bound by the next layer's claim.  Returns the point."""
        last = self.verify_rounds(claim0, t["messages"], t["challenges"], points, layer)
        point = self.point_of(t["challenges"], TRAILING)
        if not same(t["eq_r"], self.eq_eval(z, point)):
            raise Rejected(None, EQ, layer)
        if not same(last, self.mul(t["eq_r"], g_of(t["finals"]))):
            raise Rejected(None, CLAIM, layer)
        return point

    def _same_point(self, a, b):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))

    def line(self, lo, hi, tau):
        """lo + tau (hi - lo): the extension in the top variable of a table whose lower half gave lo and whose upper half gave hi"""
        return self.add(lo, self.mul(tau, self.sub(hi, lo)))

    # ---- the trees --------------------------------------------------------------------------------------------------------------------
    # Layer 0 is the 2^nv leaves; node i of layer k is made of the nodes i and i + 2^(nv - k) of layer k - 1, which are the lower and the
    # upper half of that layer: its top variable tells them apart.  `top` is layer nv - 1, two nodes, as the prover sends it; layers is
    # a dict k -> transcript for k = nv - 1 down to stop + 1, each {"z", "messages", "challenges", "finals", "eq_r", "tau"} (and
    # "lam" in a fraction tree): the claim of layer k at z is reduced to a claim of layer k - 1 at (point, tau).  The last claim is
    # checked against layer `stop` written out from the leaves by the definition of a node.
    def product_layer(self, leaves, nv, k):
        """layer k of the product tree over the leaves padded with one(): node i is the product of the leaves i + t 2^(nv - k)"""
        full = list(leaves) + [self.one] * ((1 << nv) - len(leaves))
        size = 1 << (nv - k)
        return [self.prod(full[i + t * size] for t in range(1 << k)) for i in range(size)]

    def verify_product_tree(self, leaves, nv, top, z_top, layers, stop=0):
        assert len(top) == 2 and len(z_top) == 1 and 0 <= stop < nv
        if not same(self.mul(top[0], top[1]), self.prod(leaves)):
            raise Rejected(None, ROOT, nv)
        z, claim = list(z_top), self.line(top[0], top[1], z_top[0])
        for k in range(nv - 1, stop, -1):
            t = layers[k]
            if not self._same_point(t["z"], z):
                raise Rejected(None, POINT, k)
            point = self._layer(claim, z, t, lambda f: self.mul(f[0], f[1]), 4, k)
            lo, hi = t["finals"]
            claim, z = self.line(lo, hi, t["tau"]), point + [t["tau"]]
        if not same(claim, self.mle_eval(self.product_layer(leaves, nv, stop), z)):
            raise Rejected(None, LEAVES, stop)
        return z

    def fraction_node(self, a, b):
        """(p, q) of the node over the children a and b: p_a q_b + p_b q_a, q_a q_b"""
        return self.add(self.mul(a[0], b[1]), self.mul(b[0], a[1])), self.mul(a[1], b[1])

    def fraction_layer(self, p_leaves, q_leaves, nv, k):
        """layer k of the fraction tree, as (numerators, denominators), over the leaves padded with (zero(), one()); p_leaves None:
        every stored numerator is one().  Node i sums the fractions i + t 2^(nv - k): q = prod_t q_t, p = sum_t p_t prod_{s != t} q_s"""
        n, full = len(q_leaves), 1 << nv
        ps = (list(p_leaves) if p_leaves is not None else [self.one] * n) + [self.zero] * (full - n)
        qs = list(q_leaves) + [self.one] * (full - n)
        size = 1 << (nv - k)
        P, Q = [], []
        for i in range(size):
            idx = [i + t * size for t in range(1 << k)]
            Q.append(self.prod(qs[s] for s in idx))
            P.append(self.sum(self.mul(ps[t], self.prod(qs[s] for s in idx if s != t)) for t in idx))
        return P, Q

    def verify_fraction_tree(self, p_leaves, q_leaves, nv, top, z_top, layers, stop=0):
        """top: ((p_a, q_a), (p_b, q_b)).  Returns (the last point, the root (P, Q) from the definition)."""
        assert len(top) == 2 and len(z_top) == 1 and 0 <= stop < nv
        (P,), (Q,) = self.fraction_layer(p_leaves, q_leaves, nv, nv)
        rp, rq = self.fraction_node(top[0], top[1])
        if not (same(rp, P) and same(rq, Q)):
            raise Rejected(None, ROOT, nv)
        z = list(z_top)
        pc, qc = self.line(top[0][0], top[1][0], z[0]), self.line(top[0][1], top[1][1], z[0])
        for k in range(nv - 1, stop, -1):
            t = layers[k]
            if not self._same_point(t["z"], z):
                raise Rejected(None, POINT, k)
            lam = t["lam"]
            g_of = lambda f: self.add(self.add(self.mul(f[0], f[3]), self.mul(f[1], f[2])), self.mul(lam, self.mul(f[2], f[3])))  # noqa: E731
            point = self._layer(self.add(pc, self.mul(lam, qc)), z, t, g_of, 4, k)
            p_lo, p_hi, q_lo, q_hi = t["finals"]
            pc, qc, z = self.line(p_lo, p_hi, t["tau"]), self.line(q_lo, q_hi, t["tau"]), point + [t["tau"]]
        pl, ql = self.fraction_layer(p_leaves, q_leaves, nv, stop)
        if not (same(pc, self.mle_eval(pl, z)) and same(qc, self.mle_eval(ql, z))):
            raise Rejected(None, LEAVES, stop)
        return z, (P, Q)

    # ---- the range polynomial ---------------------------------------------------------------------------------------------------------
    def range_poly(self, x, B):
        """prod_{j = -(B - 1)}^{B - 1} (x - R::from(j)): all 2 B - 1 factors"""
        return self.prod(self.sub(x, self.scalar(j)) for j in range(-(B - 1), B))
