"""Pure-Python restatement of the dense multilinear-extension folds of crates/poly, one variable at a time, generic over the
element type: the caller supplies add, sub and mul (`r * a`), so the same code runs on Python integers modulo a prime
(tests/test_mle_host.py pins it against the closed form sum_i eq(point, i) evals[i]) and on ring elements held as numpy
arrays (the expected values of tests/test_mle_gpu.py).  No kernel, no library call.

  fix_variables        mle/dense.rs:171-199                              self[b] = self[2b] + r * (self[2b+1] - self[2b])
  fix_last_variables   polynomials/multilinear_polynomial.rs:227-286     self[b] = self[b] + r * (self[b+half] - self[b])
"""
LEADING, TRAILING = 0, 1


def pad(evals, num_vars, zero):
    """the truncated storage written out (dense.rs:397-407: indexing past the stored length yields zero)"""
    assert len(evals) <= 1 << num_vars
    return list(evals) + [zero] * ((1 << num_vars) - len(evals))


def fix_variables(table, num_vars, point, add, sub, mul):
    """dense.rs:181-193: point[i] fixes variable i, the least significant index bit first"""
    t = list(table)
    assert len(t) == 1 << num_vars and len(point) <= num_vars
    for i, r in enumerate(point, start=1):
        t = [add(t[b << 1], mul(r, sub(t[(b << 1) + 1], t[b << 1]))) for b in range(1 << (num_vars - i))]
    return t


def fix_last_variables(table, num_vars, point, add, sub, mul):
    """multilinear_polynomial.rs:251-286: point[j] fixes variable num_vars - len(point) + j; the last entry is applied first"""
    t = list(table)
    assert len(t) == 1 << num_vars and len(point) <= num_vars
    nv = num_vars
    for r in reversed(point):
        half = 1 << (nv - 1)
        t = [add(t[b], mul(r, sub(t[b + half], t[b]))) for b in range(half)]
        nv -= 1
    return t


def fold(table, num_vars, point, order, add, sub, mul):
    return (fix_variables if order == LEADING else fix_last_variables)(table, num_vars, point, add, sub, mul)


def eq_closed_form(table, num_vars, point, first_var, p):
    """Prime field only: sum over the fixed bits x of prod_j (x_j point[j] + (1 - x_j)(1 - point[j])) * table[index], the fixed
    variables being first_var .. first_var + len(point) - 1.  Returns the table over the remaining variables (in index order)."""
    nf = len(point)
    rest = num_vars - nf
    out = []
    for y in range(1 << rest):
        lo, hi = y & ((1 << first_var) - 1), y >> first_var
        acc = 0
        for x in range(1 << nf):
            w = 1
            for j in range(nf):
                w = w * (point[j] if (x >> j) & 1 else (1 - point[j])) % p
            acc = (acc + w * table[lo | (x << first_var) | (hi << (first_var + nf))]) % p
        out.append(acc)
    return out
