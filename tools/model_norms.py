"""The norms of a coefficient slice in Python integers: the oracle of tests/test_norms_gpu.py.

A restatement of the reference, nothing more:
  WithLinfNorm::linf_norm / WithL2Norm::l2_norm_squared for [Fq] and Vec<Fq>    crates/ring/src/traits.rs:6-36
  per element, |signed representative| and its square                          balanced_decomposition/convertible_ring.rs:49-66
  the signed representative: x if x <= (p - 1) / 2, else x - p                   fq_convertible.rs:20-34, stark_prime/decomposition.rs:40-52
`xs` are standard-form integers in [0, p) (oracle_lib.from_mont of the memory image).
"""


def signed(x, p):
    return x if x <= (p - 1) // 2 else x - p


def linf(xs, p):
    return max(abs(signed(x, p)) for x in xs)   # an empty slice raises, as max().unwrap() panics


def l2sq(xs, p):
    return sum(signed(x, p) ** 2 for x in xs)


def groups(xs, group):
    assert group >= 1 and len(xs) % group == 0
    return [xs[i:i + group] for i in range(0, len(xs), group)]


def words(value, n):
    """little-endian u64 words of a non-negative integer that fits n of them"""
    assert 0 <= value < 1 << (64 * n)
    return [(value >> (64 * i)) & (2**64 - 1) for i in range(n)]


def records(xs, p, group, which, limbs):
    """the output of sr_norm_batch*: per group the linf words (`limbs`), then the l2sq words (3 for one limb, 9 for four)"""
    out = []
    for g in (groups(xs, group) if xs else [[]]):
        if which & 1:
            out += words(linf(g, p), limbs)
        if which & 2:
            out += words(l2sq(g, p), 3 if limbs == 1 else 9)
    return out
