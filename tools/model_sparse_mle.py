"""Pure-Python restatement of the sparse multilinear extension of crates/poly (src/mle/sparse.rs), generic over the element type:
the caller supplies add, sub and mul and the elements zero and one, so the same code runs on Python integers modulo a prime
(tests/test_smle_host.py pins it against the closed form) and on ring elements held as numpy arrays (the expected values of
tests/test_smle_gpu.py).  No kernel, no library call.  It keeps the reference's own windowing, window = max(1, ceil_log2(nnz)),
and its map keyed by index.

  precompute_eq    sparse.rs:381-394    dp[b] = prod_i (bit i of b ? g[i] : 1 - g[i]), by the doubling recurrence
  fix_variables    sparse.rs:170-207    result[idx >> w] += pre[idx & mask] * value, one window of the point at a time
  evaluate         sparse.rs:53-56      fixed_variables(point)[0]
  from_matrix      sparse.rs:97-115     index = row * next_pow2(ncols) + col, num_vars = log2(next_pow2(nrows) * next_pow2(ncols))
"""


def ceil_log2(n):
    """ark_std::log2: ceil(log2(n)), 0 for n <= 1"""
    return 0 if n <= 1 else (n - 1).bit_length()


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


def precompute_eq(g, sub, mul, one):
    """sparse.rs:381-394; an empty g gives [one] (the reference never calls it with one)"""
    if not g:
        return [one]
    dp = [None] * (1 << len(g))
    dp[0] = sub(one, g[0])
    dp[1] = g[0]
    for i in range(1, len(g)):
        for b in range(1 << i):
            prev = dp[b]
            dp[b + (1 << i)] = mul(prev, g[i])
            dp[b] = sub(prev, dp[b + (1 << i)])
    return dp


def eq_product(g, b, sub, mul, one):
    """the closed form of one entry of precompute_eq"""
    acc = one
    for i, gi in enumerate(g):
        acc = mul(acc, gi if (b >> i) & 1 else sub(one, gi))
    return acc


def fix_variables(evaluations, num_vars, point, add, sub, mul, zero, one):
    """sparse.rs:170-207.  evaluations: dict index -> element.  Returns (dict, num_vars - len(point)); entries whose sum is zero stay."""
    assert len(point) <= num_vars, "invalid partial point dimension"
    window = max(1, ceil_log2(len(evaluations)))
    last = dict(evaluations)
    rest = list(point)
    while rest:
        focus, rest = rest[:window], rest[window:]
        pre = precompute_eq(focus, sub, mul, one)
        dim = len(focus)
        result = {}
        for old_idx, value in last.items():
            new_idx = old_idx >> dim
            result[new_idx] = add(result.get(new_idx, zero), mul(pre[old_idx & ((1 << dim) - 1)], value))
        last = result
    return dict(sorted(last.items())), num_vars - len(point)


def evaluate(evaluations, num_vars, point, add, sub, mul, zero, one):
    """sparse.rs:53-56 with Index (359-365): entry 0 of the fully fixed map, zero where nothing is stored"""
    assert len(point) == num_vars
    return fix_variables(evaluations, num_vars, point, add, sub, mul, zero, one)[0].get(0, zero)


def fix_pattern(indices, n_fixed):
    """the keys of fix_variables in ascending order and the boundaries of their runs in the ascending index list"""
    keys, seg = [], []
    for j, i in enumerate(indices):
        if not keys or keys[-1] != i >> n_fixed:
            keys.append(i >> n_fixed)
            seg.append(j)
    return keys, seg + [len(indices)]


def from_matrix(rows, nrows, ncols):
    """sparse.rs:97-115.  rows: per row a list of (value, col).  Returns (num_vars, dict index -> value)."""
    n_cols = next_pow2(ncols)
    ev = {}
    for r, row in enumerate(rows):
        for value, col in row:
            ev[r * n_cols + col] = value
    return ceil_log2(next_pow2(nrows) * n_cols), ev


def matrix_cast(m):
    """the test helper of sparse.rs:431-449: the non-zero entries of a dense integer matrix, row by row"""
    return [[(v, c) for c, v in enumerate(row) if v != 0] for row in m], len(m), len(m[0])
