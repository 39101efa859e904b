"""Pure-Python restatement of the batch inversion (sr_inverse_batch, csrc/inverse.hpp), generic over the element type like the other
tools/model_*.py -- the caller supplies zero, one and mul, so the same code runs on Python integers modulo a prime, and on tuples of
them with an extension-field product (fq3_model below).  No kernel, no library call.

    out[e] = num[e] * den[e]^-1        e < n        (num None: one())

batch_inverse() is the walk of one lane over its unit: chunks of `chunk` consecutive elements, per chunk a forward walk of prefix
products, ONE inversion of the chunk's product and a backward walk.  A zero enters the products as one, leaves as zero (with or without
a numerator) and is counted.  The inversion is x^(|F| - 2) along the fixed chain of the kernel (chain()): the first two functions below.

FIELDS holds |F| of the six slot fields, CHUNKS the chunk lengths that were compiled (tools/ubench/inverse_isa.hip) with the chosen one
first; op_table() gives the products per unit of every (family, chunk): the figures of DESIGN_APPENDIX.md A.20.

`python tools/model_inverse.py` prints the chains' product counts and the table.
"""

RUN = 8  # csrc/inverse.hpp: kRun

GOLDILOCKS_P = 2**64 - 2**32 + 1
BABYBEAR_P = 2013265921
STARK_P = 2**251 + 17 * 2**192 + 1
FROG_P = 15912092521325583641
# family -> |F| of the slot field: the base field of the power-of-two rings, Fq3 / Fq9 / Fq4 of the reference's own rings
FIELDS = {"goldilocks": GOLDILOCKS_P, "babybear": BABYBEAR_P, "stark": STARK_P, "goldilocks24": GOLDILOCKS_P**3, "babybear72": BABYBEAR_P**9,
          "frog16": FROG_P**4}
RING_IDS = {"goldilocks": 0, "babybear": 1, "stark": 2, "goldilocks24": 3, "babybear72": 4, "frog16": 5}
# family -> (chunk without numerators, chunk with numerators), as csrc/inverse.hpp: kChunk
CHOSEN = {"goldilocks": (8, 4), "babybear": (8, 8), "stark": (4, 2), "goldilocks24": (4, 4), "babybear72": (2, 2), "frog16": (4, 4)}
CHUNKS = (1, 2, 4, 8, 16)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------
# A chain is a list of steps over three registers, x (the input), u and acc:
#   ("u", k)      u = u^(2^k) * u        k squarings and a product: x^(2^k - 1) -> x^(2^2k - 1); u starts as x
#   ("sq", n)     acc = acc^(2^n)        n squarings; acc starts as x
#   ("mul", "x")  acc = acc * x          ("mul", "u"): acc = acc * u
def chain(exponent, run=RUN):
    """the fixed chain of csrc/inverse.hpp: fermat() for this exponent: u = x^(2^run - 1), then the exponent from its top bit -- `run`
    set bits in a row are `run` squarings and a product by u, any other bit a squaring and, if set, a product by x"""
    assert exponent >= 1 and run & (run - 1) == 0
    steps = []
    k = 1
    while k < run:
        steps.append(("u", k))
        k *= 2
    pos = exponent.bit_length() - 2
    full = (1 << run) - 1
    while pos >= 0:
        if pos >= run - 1 and (exponent >> (pos - run + 1)) & full == full:
            steps += [("sq", run), ("mul", "u")]
            pos -= run
        else:
            steps.append(("sq", 1))
            if (exponent >> pos) & 1:
                steps.append(("mul", "x"))
            pos -= 1
    return steps


def chain_exponent(steps):
    """the exponent a chain computes, by integer bookkeeping on the exponents of its registers (x = 1)"""
    u, acc = 1, 1
    for op, arg in steps:
        if op == "u":
            u = u * (1 << arg) + u
        elif op == "sq":
            acc <<= arg
        else:
            acc += u if arg == "u" else 1
    return acc


def chain_products(steps):
    """products of the chain, squarings included"""
    return sum(arg + 1 if op == "u" else arg if op == "sq" else 1 for op, arg in steps)


def run_chain(steps, x, mul):
    u, acc = x, x
    for op, arg in steps:
        if op == "u":
            t = u
            for _ in range(arg):
                t = mul(t, t)
            u = mul(u, t)
        elif op == "sq":
            for _ in range(arg):
                acc = mul(acc, acc)
        else:
            acc = mul(acc, u if arg == "u" else x)
    return acc


def square_and_multiply_products(exponent):
    """what the plain left-to-right binary method takes for the same exponent"""
    return exponent.bit_length() - 1 + bin(exponent).count("1") - 1


# ---- the walk --------------------------------------------------------------------------------------------------------------------
def batch_inverse(den, num, chunk, order, zero, one, mul):
    """den: a list of n elements of a field of `order` elements; num: None or n elements.  -> (out, zeros): out[e] = num[e] / den[e],
    zero where den[e] is zero; zeros: how many were.  One inversion (run_chain on order - 2) per chunk, none shared between chunks."""
    assert chunk >= 1 and (num is None or len(num) == len(den))
    steps = chain(order - 2)
    n = len(den)
    out, zeros = [None] * n, 0
    for e0 in range(0, n, chunk):
        c = min(chunk, n - e0)
        x, isz = [], []
        for i in range(c):
            z = den[e0 + i] == zero
            isz.append(z)
            zeros += z
            x.append(one if z else den[e0 + i])       # the select
        pre, acc = [None] * c, x[0]
        for i in range(1, c):
            pre[i] = acc                               # x_0 ... x_(i-1)
            acc = mul(acc, x[i])
        inv = run_chain(steps, acc, mul)
        for i in range(c - 1, -1, -1):
            o = inv
            if i > 0:
                o = mul(o, pre[i])
                inv = mul(inv, x[i])
            if num is not None:
                o = mul(o, num[e0 + i])
            out[e0 + i] = zero if isz[i] else o
    return out, zeros


def direct_inverse(den, num, order, zero, one, mul):
    """element by element, by square-and-multiply on order - 2: the second formulation"""
    out, zeros = [], 0
    for e, d in enumerate(den):
        if d == zero:
            out.append(zero)
            zeros += 1
            continue
        r, b, k = one, d, order - 2
        while k:
            if k & 1:
                r = mul(r, b)
            b = mul(b, b)
            k >>= 1
        out.append(r if num is None else mul(r, num[e]))
    return out, zeros


def walk_products(chunk, has_num, inversion):
    """products of one full chunk: the forward walk, the inversion, the backward walk"""
    return (chunk - 1) + inversion + 2 * (chunk - 1) + (chunk if has_num else 0)


def op_table():
    """{(family, chunk, has_num): products per unit}"""
    t = {}
    for fam, order in FIELDS.items():
        inv = chain_products(chain(order - 2))
        for c in CHUNKS:
            for hn in (False, True):
                t[fam, c, hn] = walk_products(c, hn, inv) / c
    return t


# ---- models of the element types --------------------------------------------------------------------------------------------------
def prime_model(p):
    """(order, zero, one, mul) of Z_p"""
    return p, 0, 1, lambda a, b: a * b % p


def fq3_model(p, nonresidue):
    """(order, zero, one, mul) of Fq3 = Fq[u] / (u^3 - nonresidue) on tuples (c0, c1, c2): the slot field of goldilocks24"""
    def mul(x, y):
        c = [0] * 5
        for i in range(3):
            for j in range(3):
                c[i + j] += x[i] * y[j]
        return ((c[0] + nonresidue * c[3]) % p, (c[1] + nonresidue * c[4]) % p, c[2] % p)

    return p**3, (0, 0, 0), (1, 0, 0), mul


if __name__ == "__main__":
    for fam, order in FIELDS.items():
        s = chain(order - 2)
        assert chain_exponent(s) == order - 2
        print("%-13s |F| - 2 has %3d bits: chain %3d products, square-and-multiply %3d" %
              (fam, (order - 2).bit_length(), chain_products(s), square_and_multiply_products(order - 2)))
    t = op_table()
    print("products per unit, without / with numerators (chosen chunks marked *)")
    for fam in FIELDS:
        print("%-13s" % fam + "".join("  C=%-2d %6.1f%s/%6.1f%s" % (c, t[fam, c, False], "*" if CHOSEN[fam][0] == c else " ", t[fam, c, True],
                                                                "*" if CHOSEN[fam][1] == c else " ") for c in CHUNKS))
