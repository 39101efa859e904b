"""Host-side mirror of the reference's ring interface, at batch granularity, over the C ABI.

Reference surface mirrored (crates/ring/src/cyclotomic_ring/):
  CyclotomicConfig<N>                      ring_config.rs:11-35   -> CyclotomicRing (one per ring + degree)
    reduce_in_place                        ring_config.rs:23      -> CyclotomicRing.reduce
    crt_in_place / crt                     ring_config.rs:27,29   -> CyclotomicRing.elementwise_crt
    icrt_in_place / icrt                   ring_config.rs:30,34   -> CyclotomicRing.elementwise_icrt
  CRT::elementwise_crt / ICRT::elementwise_icrt   crt.rs:10-25, 34-49 (in place, same allocation)
  RqNTT * RqNTT (MulAssign)                ntt_form.rs:159-225    -> CyclotomicRing.ntt_mul
  RqPoly * RqPoly                          coeff_form.rs:250-258  -> CyclotomicRing.mul
  Flatten::flatten_to_coeffs / promote_from_coeffs   flatten.rs:10-34 -> same names

Buffers are numpy uint64 arrays (host entry points) or torch uint64/int64 CUDA tensors (device
entry points), in the reference's in-memory layout: element-major, D coefficients per element,
N little-endian u64 limbs per coefficient, Montgomery residues.

Errors: the reference panics on wrong lengths (e.g. goldilocks/ntt.rs:136); here RingError is raised.
"""
import ctypes

import numpy as np

from . import _lib

GOLDILOCKS_POW2, BABYBEAR_POW2, STARK_POW2, GOLDILOCKS_24, BABYBEAR_72, FROG_16 = 0, 1, 2, 3, 4, 5
PROF_TAGS = ("fwd_cols", "rows", "inv_cols", "pointwise", "other")
MLE_LEADING, MLE_TRAILING = 0, 1   # SR_MLE_LEADING / SR_MLE_TRAILING: which end of the index a fold starts from
MLE_ROUND_SUM = 2                  # SR_MLE_ROUND_SUM: the plain sum of products of sr_mle_round_evals
NORM_LINF, NORM_L2SQ = 1, 2        # SR_NORM_LINF / SR_NORM_L2SQ: the mask of sr_norm_batch*

_RING_NAMES = {
    "goldilocks": GOLDILOCKS_POW2,
    "babybear": BABYBEAR_POW2,
    "stark": STARK_POW2,
    "goldilocks24": GOLDILOCKS_24,
    "babybear72": BABYBEAR_72,
    "frog16": FROG_16,          # X^16 + 1 over the frog prime, 4 x Fq4 (frog_ring/mod.rs:62-107)
}


# BaseFieldConfig moduli: goldilocks/mod.rs:20-24, babybear/mod.rs:21-25, stark_prime/mod.rs:20-24, frog_ring/mod.rs:19-25
_MODULUS = {
    GOLDILOCKS_POW2: 2**64 - 2**32 + 1, GOLDILOCKS_24: 2**64 - 2**32 + 1,
    BABYBEAR_POW2: 2013265921, BABYBEAR_72: 2013265921,
    STARK_POW2: 2**251 + 17 * 2**192 + 1,
    FROG_16: 15912092521325583641,
}


class RingError(RuntimeError):
    pass


def _np_ptr(a):
    if not (isinstance(a, np.ndarray) and a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]):
        raise RingError("expected a C-contiguous numpy uint64 array")
    return a.ctypes.data_as(_lib.u64p)


# SR_SMLE_WINDOW_BITS / SR_SMLE_TABLE_MIN_NNZ / SR_SMLE_MAX_TABLE_ELEMS: the published constants of the sparse-MLE plan
SMLE_WINDOW_BITS, SMLE_TABLE_MIN_NNZ, SMLE_MAX_TABLE_ELEMS = 8, 1024, 2048


def smle_plan(ring, log2_degree, nnz, n_out, n_fixed):
    """sr_smle_plan: (work_elems, launches) of a sparse fold of nnz entries in n_out runs -- host arithmetic, no device, no context."""
    if isinstance(ring, str):
        ring = _RING_NAMES[ring]
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    rc = _lib.load().sr_smle_plan(int(ring), int(log2_degree), int(nnz), int(n_out), int(n_fixed), ctypes.byref(work), ctypes.byref(launches))
    if rc != 0:
        raise RingError("sr_smle_plan failed (%d): %s" % (rc, _lib.last_error()))
    return work.value, launches.value


def smle_fix_pattern(idx, num_vars, n_fixed):
    """sr_smle_fix_pattern: (out_idx, seg_ptr) -- the distinct keys idx >> n_fixed in ascending order and the run boundaries
    (len(out_idx) + 1 entries) of a strictly ascending uint64 index array; validates idx.  Host arithmetic, no device, no context."""
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    nnz = idx.size
    out_idx, seg = np.empty(max(nnz, 1), dtype=np.uint64), np.empty(nnz + 1, dtype=np.uint64)
    n_out = ctypes.c_size_t()
    if num_vars < 0 or n_fixed < 0:
        raise RingError("smle: negative count")
    rc = _lib.load().sr_smle_fix_pattern(_np_ptr(idx if nnz else out_idx), nnz, int(num_vars), int(n_fixed), _np_ptr(out_idx), _np_ptr(seg),
                                         ctypes.byref(n_out))
    if rc != 0:
        raise RingError("sr_smle_fix_pattern failed (%d): %s" % (rc, _lib.last_error()))
    return out_idx[:n_out.value].copy(), seg[:n_out.value + 1].copy()


def _log2_degree_arg(ring, log2_degree):
    return int(log2_degree) if ring <= STARK_POW2 else 0


def gram_plan(ring, log2_degree, n, m):
    """sr_gram_plan: (work_elems, launches) of the Gram matrix of an n x m matrix -- host arithmetic, no device, no context."""
    if isinstance(ring, str):
        ring = _RING_NAMES[ring]
    if n < 0 or m < 0:
        raise RingError("gram: negative count")
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    rc = _lib.load().sr_gram_plan(int(ring), _log2_degree_arg(ring, log2_degree), int(n), int(m), ctypes.byref(work), ctypes.byref(launches))
    if rc != 0:
        raise RingError("sr_gram_plan failed (%d): %s" % (rc, _lib.last_error()))
    return work.value, launches.value


def symm_recompose_plan(ring, log2_degree, n, d):
    """sr_symm_recompose_plan: (work_elems, launches) of G^T M G for a packed matrix of size n * d -- host arithmetic only."""
    if isinstance(ring, str):
        ring = _RING_NAMES[ring]
    if n < 0 or d < 0:
        raise RingError("symm_recompose: negative count")
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    rc = _lib.load().sr_symm_recompose_plan(int(ring), _log2_degree_arg(ring, log2_degree), int(n), int(d), ctypes.byref(work),
                                            ctypes.byref(launches))
    if rc != 0:
        raise RingError("sr_symm_recompose_plan failed (%d): %s" % (rc, _lib.last_error()))
    return work.value, launches.value


def _idx(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a, ctypes.c_void_p(a.ctypes.data if a.size else 0)


def _csr_args(cols, row_ptr, nrows, what):
    if nrows < 0:
        raise RingError("%s: negative count" % what)
    row_ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    if row_ptr.size != nrows + 1:
        raise RingError("%s: row_ptr must have nrows + 1 entries" % what)
    cols = np.ascontiguousarray(cols, dtype=np.uint32)
    if cols.size != int(row_ptr[-1]):
        raise RingError("%s: cols must have row_ptr[nrows] entries" % what)
    return cols, row_ptr


def sparse_transpose_pattern(cols, row_ptr, nrows, ncols):
    """sr_sparse_transpose_pattern: (t_row_ptr, t_cols, perm) of the transpose of a CSR pattern -- a stable counting sort by column,
    t_vals[t] = vals[perm[t]].  Host arithmetic, no device, no context."""
    if ncols < 0:
        raise RingError("sparse_transpose_pattern: negative count")
    cols, row_ptr = _csr_args(cols, row_ptr, nrows, "sparse_transpose_pattern")
    t_row_ptr = np.empty(ncols + 1, dtype=np.uint64)
    t_cols, perm = np.empty(cols.size, dtype=np.uint32), np.empty(cols.size, dtype=np.uint32)
    rc = _lib.load().sr_sparse_transpose_pattern(_idx(cols, np.uint32)[1], row_ptr.ctypes.data, nrows, ncols, t_row_ptr.ctypes.data,
                                                 _idx(t_cols, np.uint32)[1], _idx(perm, np.uint32)[1])
    if rc != 0:
        raise RingError("sr_sparse_transpose_pattern failed (%d): %s" % (rc, _lib.last_error()))
    return t_row_ptr, t_cols, perm


def spgemm_pattern(a_cols, a_row_ptr, n, m, b_cols, b_row_ptr, p, count_only=False):
    """sr_spgemm_pattern: the structural product of two CSR patterns with strictly ascending rows -- (out_row_ptr, out_cols, pair_ptr,
    pair_a, pair_b), or (n_out, n_pairs) with count_only.  Host arithmetic, no device, no context."""
    if m < 0 or p < 0:
        raise RingError("spgemm_pattern: negative count")
    a_cols, a_row_ptr = _csr_args(a_cols, a_row_ptr, n, "spgemm_pattern")
    b_cols, b_row_ptr = _csr_args(b_cols, b_row_ptr, m, "spgemm_pattern")
    lib = _lib.load()
    n_out, n_pairs = ctypes.c_size_t(), ctypes.c_size_t()
    head = (_idx(a_cols, np.uint32)[1], a_row_ptr.ctypes.data, n, m, _idx(b_cols, np.uint32)[1], b_row_ptr.ctypes.data, p)
    rc = lib.sr_spgemm_pattern(*head, None, None, None, None, None, ctypes.byref(n_out), ctypes.byref(n_pairs))
    if rc != 0:
        raise RingError("sr_spgemm_pattern failed (%d): %s" % (rc, _lib.last_error()))
    if count_only:
        return n_out.value, n_pairs.value
    out_row_ptr, pair_ptr = np.empty(n + 1, dtype=np.uint64), np.empty(n_out.value + 1, dtype=np.uint64)
    out_cols = np.empty(n_out.value, dtype=np.uint32)
    pair_a, pair_b = np.empty(n_pairs.value, dtype=np.uint32), np.empty(n_pairs.value, dtype=np.uint32)
    rc = lib.sr_spgemm_pattern(*head, out_row_ptr.ctypes.data, _idx(out_cols, np.uint32)[1], pair_ptr.ctypes.data, _idx(pair_a, np.uint32)[1],
                               _idx(pair_b, np.uint32)[1], ctypes.byref(n_out), ctypes.byref(n_pairs))
    if rc != 0:
        raise RingError("sr_spgemm_pattern failed (%d): %s" % (rc, _lib.last_error()))
    return out_row_ptr, out_cols, pair_ptr, pair_a, pair_b


def spgemm_plan(ring, log2_degree, n_out, n_pairs):
    """sr_spgemm_plan: (work_elems, launches) of the numeric phase of a sparse product -- host arithmetic, no device, no context."""
    if isinstance(ring, str):
        ring = _RING_NAMES[ring]
    if n_out < 0 or n_pairs < 0:
        raise RingError("spgemm: negative count")
    work, launches = ctypes.c_size_t(), ctypes.c_int()
    rc = _lib.load().sr_spgemm_plan(int(ring), _log2_degree_arg(ring, log2_degree), int(n_out), int(n_pairs), ctypes.byref(work),
                                    ctypes.byref(launches))
    if rc != 0:
        raise RingError("sr_spgemm_plan failed (%d): %s" % (rc, _lib.last_error()))
    return work.value, launches.value


def _basis_words(basis, decompose):
    """(lo, hi) 64-bit words of a decomposition basis (the reference takes b: u128, balanced_decomposition/mod.rs:62).  Anything
    outside [0, 2^128) is refused instead of being truncated by ctypes.  decompose_balanced_in_place casts `b as i128` (mod.rs:73),
    so a basis of 2^127 or more would be a NEGATIVE basis there; that case is refused here (and by the C ABI) rather than computed
    with unsigned semantics the reference does not have.  Recomposition (`R::from(b)`, mod.rs:105-117) has no such cast."""
    basis = int(basis)
    if not 0 <= basis < 1 << 128:
        raise RingError("basis out of the u128 range")
    if decompose and basis >= 1 << 127:
        raise RingError("basis >= 2^127: negative after the reference's `b as i128` (balanced_decomposition/mod.rs:73); not supported")
    return basis & (2**64 - 1), basis >> 64


class CyclotomicRing:
    """One ring configuration bound to one HIP device (the analogue of a `CyclotomicConfig` impl)."""

    def __init__(self, ring, log2_degree=0, device=0, plan=None):
        """plan: a _lib.Plan (sr_plan); None = the SR_* switches of the environment as parsed by _lib.plan_from_env (all unset =
        the library defaults).  The library itself never reads the environment."""
        if isinstance(ring, str):
            ring = _RING_NAMES[ring]
        self._lib = _lib.load()
        self._ctx = ctypes.c_void_p()
        if plan is None:
            plan = _lib.plan_from_env(int(ring))
        self.plan = plan
        rc = self._lib.sr_ctx_create_ex(int(ring), int(log2_degree), int(device), ctypes.byref(plan), ctypes.byref(self._ctx))
        if rc != 0:
            self._ctx = None
            raise RingError("sr_ctx_create_ex failed (%d): %s" % (rc, _lib.last_error()))
        self.ring = int(ring)
        self.device = int(device)
        d = ctypes.c_size_t()
        l = ctypes.c_int()
        self._check(self._lib.sr_ctx_degree(self._ctx, ctypes.byref(d)))
        self._check(self._lib.sr_ctx_limbs(self._ctx, ctypes.byref(l)))
        self.degree = d.value          # PolyRing::dimension()
        self.limbs = l.value           # N
        self.words_per_elem = self.degree * self.limbs
        self.modulus = _MODULUS[self.ring]

    # -- lifetime --------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.sr_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise RingError("stark_rings_hip call failed (%d): %s" % (rc, _lib.last_error()))

    def _batch_of(self, arr_words):
        if arr_words % self.words_per_elem != 0:
            # promote_from_coeffs returns None in the reference (flatten.rs:22-24); transforms panic
            raise RingError("buffer length %d is not a multiple of D*N = %d" % (arr_words, self.words_per_elem))
        return arr_words // self.words_per_elem

    # -- Flatten (flatten.rs:10-34): zero-copy views ---------------------------------------------
    def flatten_to_coeffs(self, elems):
        """(batch, D[, N]) -> flat view of batch*D coefficients."""
        return elems.reshape(-1, self.limbs) if self.limbs > 1 else elems.reshape(-1)

    def promote_from_coeffs(self, flat):
        """flat coefficients -> (batch, D[, N]) view, or None if the length is not a multiple of D."""
        n = flat.size if isinstance(flat, np.ndarray) else flat.numel()
        if n % self.words_per_elem != 0:
            return None
        shape = (n // self.words_per_elem, self.degree) + ((self.limbs,) if self.limbs > 1 else ())
        return flat.reshape(shape)

    # -- host-buffer API (numpy) -----------------------------------------------------------
    def elementwise_crt(self, data):
        """CRT::elementwise_crt (crt.rs:10-25): in place on a numpy uint64 buffer."""
        self._check(self._lib.sr_ntt_fwd_batch(self._ctx, _np_ptr(data), self._batch_of(data.size)))
        return data

    def elementwise_icrt(self, data):
        """ICRT::elementwise_icrt (crt.rs:34-49): in place."""
        self._check(self._lib.sr_ntt_inv_batch(self._ctx, _np_ptr(data), self._batch_of(data.size)))
        return data

    def ntt_mul(self, lhs, rhs):
        """lhs *= rhs slot-wise in CRT form (ntt_form.rs:213-225), in place on lhs."""
        if lhs.size != rhs.size:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_pointwise_mul_batch(self._ctx, _np_ptr(lhs), _np_ptr(rhs), self._batch_of(lhs.size)))
        return lhs

    def add(self, lhs, rhs):
        """lhs += rhs element-wise (ntt_form.rs:227-285 / coeff_form.rs Add), in place on lhs."""
        if lhs.size != rhs.size:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_add_batch(self._ctx, _np_ptr(lhs), _np_ptr(rhs), self._batch_of(lhs.size)))
        return lhs

    def sub(self, lhs, rhs):
        """lhs -= rhs element-wise (ntt_form.rs:588-638), in place on lhs."""
        if lhs.size != rhs.size:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_sub_batch(self._ctx, _np_ptr(lhs), _np_ptr(rhs), self._batch_of(lhs.size)))
        return lhs

    def _scalar(self, scalar):
        """one base-field element as the library takes it: `limbs` u64 words, the Montgomery memory image of Fp::from(rhs)"""
        s = np.ascontiguousarray(np.asarray(scalar, dtype=np.uint64).reshape(-1))
        if s.size != self.limbs:
            raise RingError("scalar must be %d u64 limb(s)" % self.limbs)
        return s

    def neg(self, data):
        """Neg (coeff_form.rs:270-278, ntt_form.rs:191-203): data = -data word-wise, in place, either form."""
        self._check(self._lib.sr_neg_batch(self._ctx, _np_ptr(data), self._batch_of(data.size)))
        return data

    def scale(self, data, scalar):
        """Mul<Fp> / Mul<primitive> / MulAssign (coeff_form.rs:390-408, 610-650; ntt_form.rs:373-425): every coefficient (slot
        component) times one base-field scalar given as its Montgomery image; in place, either form."""
        s = self._scalar(scalar)
        self._check(self._lib.sr_scale_batch(self._ctx, _np_ptr(data), _np_ptr(s), self._batch_of(data.size)))
        return data

    def mul_elem(self, data, elem):
        """`Matrix<R> *= &R` / `SparseMatrix<R> *= &R` (linear_algebra/src/matrix.rs:207-211, sparse_matrix.rs:303-307) on the
        matrix's flat storage: every element of the batch (CRT/NTT form) times ONE ring element, slot-wise, in place."""
        if elem.size != self.words_per_elem:
            raise RingError("mul_elem: the multiplier is not one ring element")
        if data.size:
            self._check(self._lib.sr_mul_elem_batch(self._ctx, _np_ptr(data), _np_ptr(elem), self._batch_of(data.size)))
        return data

    def mul_elem_add(self, acc, x, r):
        """Host buffers: acc[e] += r * x[e] slot-wise (see mul_elem_add_dev), in place on acc."""
        if acc.size != x.size:
            raise RingError("operand lengths differ")
        if r.size != self.words_per_elem:
            raise RingError("mul_elem_add: the multiplier is not one ring element")
        if acc.size:
            self._check(self._lib.sr_mul_elem_add_batch(self._ctx, _np_ptr(acc), _np_ptr(x), _np_ptr(r), self._batch_of(acc.size)))
        return acc

    def mle_fix_variables(self, evals, num_vars, point, order=MLE_LEADING):
        """Host buffers: sr_mle_fix_variables (see mle_fix_variables_dev); returns the 2^(num_vars - n_fixed) folded elements."""
        n_fixed = self._batch_of(point.size)
        if n_fixed > num_vars:
            raise RingError("mle_fix_variables: the point has more entries than the table has variables")
        out = np.empty(self.words_per_elem << (num_vars - n_fixed), dtype=np.uint64)
        n_evals, n_fixed = self._mle_sizes(evals.size, num_vars, point.size, out.size)
        z = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_mle_fix_variables(self._ctx, _np_ptr(out), _np_ptr(evals if n_evals else z), n_evals, int(num_vars),
                                                   _np_ptr(point if n_fixed else z), n_fixed, int(order)))
        return out

    # -- sparse multilinear extensions (crates/poly mle/sparse.rs) ---------------------------------------------------------------------
    def eq_table(self, point):
        """Host buffers: sr_eq_table -- the 2^n eq(point, .) elements of an n-element point (precompute_eq, sparse.rs:381-394)."""
        n = self._batch_of(point.size)
        out = np.empty(self.words_per_elem << n, dtype=np.uint64)
        self._check(self._lib.sr_eq_table(self._ctx, _np_ptr(out), _np_ptr(point if n else out), n))
        return out

    def smle_fix_variables(self, vals, idx, num_vars, point):
        """Host buffers: sr_smle_fix_variables -- (out_vals, out_idx) of the sparse MLE (idx ascending, vals in the same order) with
        the first len(point) variables fixed (see smle_fix_variables_dev)."""
        idx = np.ascontiguousarray(idx, dtype=np.uint64)
        nnz, n_fixed = idx.size, self._batch_of(point.size)
        if self._batch_of(vals.size) != nnz:
            raise RingError("smle_fix_variables: one value per index")
        out_vals, out_idx = np.empty(max(nnz, 1) * self.words_per_elem, dtype=np.uint64), np.empty(max(nnz, 1), dtype=np.uint64)
        n_out = ctypes.c_size_t()
        z = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_smle_fix_variables(self._ctx, _np_ptr(out_vals), _np_ptr(out_idx), ctypes.byref(n_out), _np_ptr(vals if nnz else z),
                                                    _np_ptr(idx if nnz else z), nnz, int(num_vars), _np_ptr(point if n_fixed else z), n_fixed))
        return out_vals[:n_out.value * self.words_per_elem].copy(), out_idx[:n_out.value].copy()

    # -- norms of coefficient slices (traits.rs:6-36: WithLinfNorm / WithL2Norm over [Fq]) ---------------------------------------
    def norm_plan(self, n_coeffs, group=None, which=NORM_LINF | NORM_L2SQ):
        """sr_norm_plan: (words per group, workspace words, launches) -- host arithmetic only.  group None = the whole slice."""
        wpg, work, launches = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_int()
        self._check(self._lib.sr_norm_plan(self.ring, int(n_coeffs), self._norm_group(n_coeffs, group), int(which), ctypes.byref(wpg),
                                           ctypes.byref(work), ctypes.byref(launches)))
        return wpg.value, work.value, launches.value

    def _norm_group(self, n_coeffs, group):
        return int(group) if group is not None else max(int(n_coeffs), 1)

    def _norm_coeffs(self, n_words):
        if n_words % self.limbs:
            raise RingError("buffer length %d is not a multiple of the %d words of a coefficient" % (n_words, self.limbs))
        return n_words // self.limbs

    def _norm_ints(self, words, which, whole):
        """the records of sr_norm_batch* as Python integers: linf, l2sq or (linf, l2sq) per group; one value for the whole slice"""
        nl = self.limbs if which & NORM_LINF else 0
        ns = (3 if self.limbs == 1 else 9) if which & NORM_L2SQ else 0
        recs = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, nl + ns)
        val = lambda ws: int.from_bytes(ws.astype("<u8").tobytes(), "little")
        res = []
        for r in recs:
            parts = ([val(r[:nl])] if nl else []) + ([val(r[nl:])] if ns else [])
            res.append(parts[0] if len(parts) == 1 else tuple(parts))
        return res[0] if whole else res

    def _norm_host(self, coeffs, group, which):
        n = self._norm_coeffs(coeffs.size)
        wpg = self.norm_plan(n, group, which)[0]
        g = self._norm_group(n, group)
        out = np.empty(max(n // g, 1) * wpg, dtype=np.uint64)
        src = coeffs if n else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_norm_batch(self._ctx, _np_ptr(out), _np_ptr(src), n, g, int(which)))
        return self._norm_ints(out, which, group is None)

    def linf_norm(self, coeffs, group=None):
        """Host buffer of coefficients (flatten_to_coeffs): max |signed representative| as a Python int; group = g: a list, one per g
        consecutive coefficients.  An empty slice is refused (the reference panics)."""
        return self._norm_host(coeffs, group, NORM_LINF)

    def l2_norm_squared(self, coeffs, group=None):
        """Host buffer: the sum of the squared signed representatives, exact (see linf_norm)."""
        return self._norm_host(coeffs, group, NORM_L2SQ)

    def norms(self, coeffs, group=None):
        """Host buffer: (linf, l2sq) from one pass over the data; a list of such pairs with group = g."""
        return self._norm_host(coeffs, group, NORM_LINF | NORM_L2SQ)

    def add_scalar(self, data, scalar, ntt_form):
        """Add<primitive> (coeff_form.rs:652-700: coefficient 0 of every element; ntt_form.rs:427-505: component 0 of every slot);
        Sub: pass the negated scalar.  In place."""
        s = self._scalar(scalar)
        self._check(self._lib.sr_add_scalar_batch(self._ctx, _np_ptr(data), _np_ptr(s), 1 if ntt_form else 0, self._batch_of(data.size)))
        return data

    def sum(self, elems):
        """impl Sum for RqPoly / RqNTT (coeff_form.rs:507-521, ntt_form.rs:640-654): `iter.fold(zero(), |acc, x| acc + x)` over a slice
        of ring elements, word-wise, either form; an empty slice gives zero().  Returns one ring element."""
        out = np.empty(self.words_per_elem, dtype=np.uint64)
        src = elems if elems.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_sum_batch(self._ctx, _np_ptr(out), _np_ptr(src), self._batch_of(elems.size)))
        return out

    def product(self, elems_ntt):
        """impl Product for RqNTT (ntt_form.rs:656-670): `iter.fold(one(), |acc, x| acc * x)`, slot-wise; an empty slice gives one()."""
        out = np.empty(self.words_per_elem, dtype=np.uint64)
        src = elems_ntt if elems_ntt.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_product_batch(self._ctx, _np_ptr(out), _np_ptr(src), self._batch_of(elems_ntt.size)))
        return out

    def product_poly(self, elems):
        """impl Product for RqPoly (coeff_form.rs:523-537: `iter.fold(one(), |acc, x| acc * x)` with the ring product) as
        icrt(product(crt(x_i))): the CRT is a ring isomorphism, so the slot-wise product of the transforms is the transform of the
        product.  The input is not modified."""
        t = self.elementwise_crt(elems.copy()) if elems.size else elems
        return self.elementwise_icrt(self.product(t))

    def mul(self, a, b, out=None):
        """Coefficient-form product a * b (coeff_form.rs:250-258) via icrt(crt(a) * crt(b))."""
        if a.size != b.size:
            raise RingError("operand lengths differ")
        if out is None:
            out = np.empty_like(a)
        self._check(self._lib.sr_ring_mul_batch(self._ctx, _np_ptr(out), _np_ptr(a), _np_ptr(b), self._batch_of(a.size)))
        return out

    def matvec_ntt(self, m, v, nrows, ncols):
        """Host buffers: Matrix<RqNTT>::checked_mul_vec (matrix.rs:168-178); RingError where the reference returns None."""
        w = self.words_per_elem
        if m.size != nrows * ncols * w or v.size != ncols * w:
            raise RingError("matvec: DifferentLengths")
        y = np.empty(max(nrows * w, 1), dtype=np.uint64)[:nrows * w]
        self._check(self._lib.sr_matvec_ntt(self._ctx, _np_ptr(y) if nrows else _np_ptr(np.zeros(1, dtype=np.uint64)),
                                            _np_ptr(m) if m.size else _np_ptr(np.zeros(1, dtype=np.uint64)),
                                            _np_ptr(v) if v.size else _np_ptr(np.zeros(1, dtype=np.uint64)), nrows, ncols))
        return y

    def spmv_ntt(self, rows, v, ncols):
        """rows: the reference's SparseMatrix.coeffs -- a list (one per row) of lists of (ring element as uint64 words, column).
        SparseMatrix<RqNTT>::checked_mul_vec (sparse_matrix.rs:201-211); an out-of-range column raises RingError (the
        reference panics on v[col])."""
        w = self.words_per_elem
        if v.size != ncols * w:
            raise RingError("spmv: DifferentLengths")
        nrows = len(rows)
        row_ptr = np.zeros(nrows + 1, dtype=np.uint64)
        for r, row in enumerate(rows):
            row_ptr[r + 1] = row_ptr[r] + len(row)
        nnz = int(row_ptr[-1])
        vals = np.zeros(max(nnz * w, 1), dtype=np.uint64)
        cols = np.zeros(max(nnz, 1), dtype=np.uint32)
        j = 0
        for row in rows:
            for elem, col in row:
                vals[j * w:(j + 1) * w] = elem
                cols[j] = col
                j += 1
        y = np.empty(max(nrows * w, 1), dtype=np.uint64)
        vv = v if v.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_spmv_ntt(self._ctx, _np_ptr(y), _np_ptr(vals), cols.ctypes.data_as(ctypes.c_void_p), _np_ptr(row_ptr), _np_ptr(vv),
                                          nrows, ncols))
        return y[:nrows * w]

    def matmul_ntt(self, a, b, n, m, p):
        """Host buffers: Matrix<RqNTT>::checked_mul_mat (matrix.rs:148-166)."""
        w = self.words_per_elem
        if a.size != n * m * w or b.size != m * p * w:
            raise RingError("matmul: DifferentLengths")
        y = np.empty(max(n * p * w, 1), dtype=np.uint64)
        z = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_matmul_ntt(self._ctx, _np_ptr(y), _np_ptr(a) if a.size else _np_ptr(z),
                                            _np_ptr(b) if b.size else _np_ptr(z), n, m, p))
        return y[:n * p * w]

    # -- symmetric matrices (linear_algebra/src/symmetric_matrix.rs; packed: entry (i, j), j <= i, is element i (i + 1) / 2 + j) ----
    def gram_ntt(self, a, n, m):
        """Host buffers: sr_gram_ntt -- the packed Gram matrix out(i, j) = sum_t a[i][t] * a[j][t] of a dense n x m matrix."""
        w = self.words_per_elem
        if n < 0 or m < 0 or a.size != n * m * w:
            raise RingError("gram: DifferentLengths")
        out = np.empty(max(n * (n + 1) // 2 * w, 1), dtype=np.uint64)
        self._check(self._lib.sr_gram_ntt(self._ctx, _np_ptr(out), _np_ptr(a if a.size else out), n, m))
        return out[:n * (n + 1) // 2 * w]

    def symm_recompose(self, mat, n, d, powers):
        """Host buffers: sr_symm_recompose -- recompose_left_right_symmetric_matrix (balanced_decomposition/mod.rs:354-386) of a
        packed matrix of size n * d with the d ring elements `powers`; returns the packed matrix of size n."""
        w = self.words_per_elem
        if n < 0 or d < 0 or powers.size != d * w or mat.size != (n * d) * (n * d + 1) // 2 * w:
            raise RingError("symm_recompose: DifferentLengths")
        out = np.empty(max(n * (n + 1) // 2 * w, 1), dtype=np.uint64)
        self._check(self._lib.sr_symm_recompose(self._ctx, _np_ptr(out), _np_ptr(mat if mat.size else out), n, d,
                                                _np_ptr(powers if powers.size else out)))
        return out[:n * (n + 1) // 2 * w]

    # -- sparse matrices: transpose and sparse x sparse product (linear_algebra/src/ops.rs:9-62, sparse_matrix.rs:219-281) --------------
    sparse_transpose_pattern = staticmethod(sparse_transpose_pattern)
    spgemm_pattern = staticmethod(spgemm_pattern)

    def _flatten_rows(self, rows):
        """the reference's SparseMatrix.coeffs (rows of (element words, column)) -> (vals, cols, row_ptr)"""
        w = self.words_per_elem
        row_ptr = np.zeros(len(rows) + 1, dtype=np.uint64)
        for r, row in enumerate(rows):
            row_ptr[r + 1] = row_ptr[r] + len(row)
        nnz = int(row_ptr[-1])
        vals, cols = np.zeros(max(nnz * w, 1), dtype=np.uint64), np.zeros(max(nnz, 1), dtype=np.uint32)
        j = 0
        for row in rows:
            for elem, col in row:
                if not 0 <= col < 1 << 32:
                    raise RingError("column index out of range")
                vals[j * w:(j + 1) * w] = elem
                cols[j] = col
                j += 1
        return vals, cols, row_ptr, nnz

    def _rows_of(self, vals, cols, row_ptr):
        w = self.words_per_elem
        return [[(vals[t * w:(t + 1) * w].copy(), int(cols[t])) for t in range(int(row_ptr[i]), int(row_ptr[i + 1]))]
                for i in range(len(row_ptr) - 1)]

    def transpose(self, data, nrows, ncols):
        """Host buffers: the data of Matrix::transpose (ops.rs:36-44) -- out[j][i] = data[i][j] for a row-major nrows x ncols matrix,
        as one flat array of ncols x nrows ring elements."""
        if nrows < 0 or ncols < 0 or data.size != nrows * ncols * self.words_per_elem:
            raise RingError("transpose: DifferentLengths")
        out = np.empty(max(data.size, 1), dtype=np.uint64)
        self._check(self._lib.sr_transpose(self._ctx, _np_ptr(out), _np_ptr(data if data.size else out), nrows, ncols))
        return out[:data.size]

    def sparse_transpose(self, rows, ncols):
        """Host buffers: SparseMatrix::transpose (ops.rs:46-62) of the len(rows) x ncols matrix whose rows are those of spmv_ntt
        (SparseMatrix.coeffs); returns the ncols rows of the result.  The rows need not be sorted."""
        w, nrows = self.words_per_elem, len(rows)
        vals, cols, row_ptr, nnz = self._flatten_rows(rows)
        t_vals, t_cols = np.zeros(max(nnz * w, 1), dtype=np.uint64), np.zeros(max(nnz, 1), dtype=np.uint32)
        t_row_ptr = np.zeros(ncols + 1, dtype=np.uint64)
        self._check(self._lib.sr_sparse_transpose(self._ctx, t_vals.ctypes.data, t_cols.ctypes.data, t_row_ptr.ctypes.data, vals.ctypes.data,
                                                  cols.ctypes.data, row_ptr.ctypes.data, nrows, ncols))
        return self._rows_of(t_vals, t_cols, t_row_ptr)

    def spgemm_ntt(self, rows_a, rows_b, m, p):
        """Host buffers: SparseMatrix<RqNTT>::checked_mul_mat (sparse_matrix.rs:219-275) of A (len(rows_a) x m) and B (m x p); the row
        lists are those of spmv_ntt.  Returns the rows of the product; RingError where the reference returns None (len(rows_b) != m)
        and for rows that do not ascend strictly."""
        if len(rows_b) != m:
            raise RingError("spgemm: DifferentLengths")
        n, w = len(rows_a), self.words_per_elem
        av, ac, ap, _ = self._flatten_rows(rows_a)
        bv, bc, bp, _ = self._flatten_rows(rows_b)
        n_out, _ = spgemm_pattern(ac[:int(ap[-1])], ap, n, m, bc[:int(bp[-1])], bp, p, count_only=True)
        out_vals, out_cols = np.zeros(max(n_out * w, 1), dtype=np.uint64), np.zeros(max(n_out, 1), dtype=np.uint32)
        out_row_ptr, nnz = np.zeros(n + 1, dtype=np.uint64), ctypes.c_size_t()
        self._check(self._lib.sr_spgemm_ntt(self._ctx, out_vals.ctypes.data, out_cols.ctypes.data, out_row_ptr.ctypes.data, ctypes.byref(nnz),
                                            av.ctypes.data, ac.ctypes.data, ap.ctypes.data, n, m, bv.ctypes.data, bc.ctypes.data, bp.ctypes.data, p))
        return self._rows_of(out_vals, out_cols, out_row_ptr)

    def rot(self, data):
        """Cyclotomic::rot (traits.rs:54-66) of every element of the batch, in place: coefficients times X modulo the ring."""
        self._check(self._lib.sr_rot_batch(self._ctx, _np_ptr(data), self._batch_of(data.size)))
        return data

    def gadget_decompose(self, a, basis, padding_size):
        """GadgetDecompose for a Vec of ring elements in coefficient form (balanced_decomposition/mod.rs:163-175): returns
        len * padding_size elements, digit j of element e at index e * padding_size + j.  RingError where the reference panics
        (basis 0, 1 or odd; more than padding_size digits needed)."""
        batch = self._batch_of(a.size)
        out = np.empty(max(batch * padding_size * self.words_per_elem, 1), dtype=np.uint64)
        src = a if a.size else np.zeros(1, dtype=np.uint64)
        lo, hi = _basis_words(basis, True)
        self._check(self._lib.sr_decompose_balanced_batch_wide(self._ctx, _np_ptr(out), _np_ptr(src), lo, hi, padding_size, batch))
        return out[:batch * padding_size * self.words_per_elem]

    def gadget_recompose(self, digits, basis, padding_size):
        """GadgetRecompose (mod.rs:177-189): len / padding_size elements, each sum_j basis^j * digits[e * padding_size + j]."""
        n = self._batch_of(digits.size)
        if padding_size == 0 or n % padding_size:
            raise RingError("recompose: length is not a multiple of padding_size")
        batch_out = n // padding_size
        out = np.empty(max(batch_out * self.words_per_elem, 1), dtype=np.uint64)
        src = digits if digits.size else np.zeros(1, dtype=np.uint64)
        lo, hi = _basis_words(basis, False)
        self._check(self._lib.sr_recompose_batch_wide(self._ctx, _np_ptr(out), _np_ptr(src), lo, hi, padding_size, batch_out))
        return out[:batch_out * self.words_per_elem]

    # -- GadgetDecompose / GadgetRecompose for Matrix<R> and SparseMatrix<R> (balanced_decomposition/mod.rs:276-352) ------------
    def matrix_gadget_decompose(self, mat, nrows, ncols, basis, padding_size):
        """Matrix<R> of nrows x ncols ring elements (row-major, coefficient form) -> nrows x (padding_size * ncols): every row
        is gadget-decomposed as a slice (mod.rs:291-296), i.e. entry (r, c) becomes entries (r, c * k .. c * k + k - 1).  Row-major
        storage makes this the batch decomposition of the flat element array.  Returns (flat words, nrows, ncols * padding_size)."""
        if mat.size != nrows * ncols * self.words_per_elem:
            raise RingError("matrix_gadget_decompose: DifferentLengths")
        return self.gadget_decompose(mat, basis, padding_size), nrows, ncols * padding_size

    def matrix_gadget_recompose(self, mat, nrows, ncols, basis, padding_size):
        """Inverse shape map (mod.rs:299-307): nrows x ncols -> nrows x (ncols / padding_size)."""
        if mat.size != nrows * ncols * self.words_per_elem or padding_size == 0 or ncols % padding_size:
            raise RingError("matrix_gadget_recompose: ncols is not a multiple of padding_size")
        return self.gadget_recompose(mat, basis, padding_size), nrows, ncols // padding_size

    def sparse_gadget_decompose(self, rows, ncols, basis, padding_size):
        """SparseMatrix<R> (rows: list of lists of (element words, column)) -> the same with ncols * padding_size columns
        (mod.rs:323-336): stored entry (e, c) becomes (digit_i(e), c * k + i) for i < k, zero digits dropped ("maintain full
        sparsity", mod.rs:208-229).  One batched device decomposition over all stored entries."""
        w = self.words_per_elem
        flat = [np.ascontiguousarray(e, dtype=np.uint64) for row in rows for e, _ in row]
        if any(e.size != w for e in flat):
            raise RingError("sparse_gadget_decompose: entry is not one ring element")
        if any(c >= ncols for row in rows for _, c in row):
            raise RingError("sparse_gadget_decompose: column out of range")
        digits = self.gadget_decompose(np.concatenate(flat) if flat else np.zeros(0, dtype=np.uint64), basis, padding_size)
        out, j = [], 0
        for row in rows:
            new = []
            for _, c in row:
                for i in range(padding_size):
                    dgt = digits[(j * padding_size + i) * w:(j * padding_size + i + 1) * w]
                    if dgt.any():               # r != R::zero(): the Montgomery image of zero is all-zero words
                        new.append((dgt.copy(), c * padding_size + i))
                j += 1
            out.append(new)
        return out, ncols * padding_size

    def sparse_gadget_recompose(self, rows, ncols, basis, padding_size):
        """mod.rs:231-266, 339-351: consecutive entries whose column / padding_size agree form one original entry; missing
        digits are zero."""
        if padding_size == 0 or ncols % padding_size:
            raise RingError("sparse_gadget_recompose: ncols is not a multiple of padding_size")
        w = self.words_per_elem
        groups, shape = [], []
        for row in rows:
            cnt, prev = 0, None
            for e, c in row:
                idx = c // padding_size
                if idx != prev:
                    groups.append((idx, np.zeros(padding_size * w, dtype=np.uint64)))
                    cnt += 1
                    prev = idx
                groups[-1][1][(c % padding_size) * w:(c % padding_size + 1) * w] = e
            shape.append(cnt)
        vals = self.gadget_recompose(np.concatenate([g[1] for g in groups]) if groups else np.zeros(0, dtype=np.uint64), basis,
                                     padding_size)
        out, j = [], 0
        for cnt in shape:
            out.append([(vals[(j + t) * w:(j + t + 1) * w].copy(), groups[j + t][0]) for t in range(cnt)])
            j += cnt
        return out, ncols // padding_size

    @property
    def wire_coeff_bytes(self):
        """Bytes per coefficient on the ark-serialize wire: 8 (Goldilocks, frog), 4 (BabyBear), 32 (Stark)."""
        return int(self._lib.sr_wire_coeff_bytes(self._ctx))

    def serialize(self, a):
        """CanonicalSerialize of every ring element of the batch (coeff_form.rs:154-189, ntt_form.rs:24): the flat coefficients as
        little-endian standard-form integers, wire_coeff_bytes each, no length prefix.  Returns a uint8 array."""
        batch = self._batch_of(a.size)
        out = np.empty(max(batch * self.degree * self.wire_coeff_bytes, 1), dtype=np.uint8)
        src = a if a.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_serialize_batch(self._ctx, out.ctypes.data_as(ctypes.c_void_p), _np_ptr(src), batch))
        return out[:batch * self.degree * self.wire_coeff_bytes]

    def deserialize(self, wire):
        """CanonicalDeserialize of a whole number of ring elements; RingError (ark: InvalidData) when a coefficient is >= p."""
        wire = np.ascontiguousarray(wire, dtype=np.uint8)
        per = self.degree * self.wire_coeff_bytes
        if wire.size % per:
            raise RingError("deserialize: not a whole number of ring elements")
        batch = wire.size // per
        out = np.empty(max(batch * self.words_per_elem, 1), dtype=np.uint64)
        src = wire if wire.size else np.zeros(8, dtype=np.uint8)
        self._check(self._lib.sr_deserialize_batch(self._ctx, _np_ptr(out), src.ctypes.data_as(ctypes.c_void_p), batch))
        return out[:batch * self.words_per_elem]

    def reduce(self, coeffs, in_len_per_elem, batch):
        """CyclotomicConfig::reduce_in_place (ring_config.rs:23): (batch, in_len) -> (batch, D)."""
        if coeffs.size != batch * in_len_per_elem * self.limbs:
            raise RingError("reduce: buffer length does not match batch * in_len")
        out = np.empty(batch * self.words_per_elem, dtype=np.uint64)
        src = coeffs if coeffs.size else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_reduce_batch(self._ctx, _np_ptr(src), in_len_per_elem, _np_ptr(out), batch))
        return out

    # -- device-resident API (torch CUDA tensors of 8-byte integers) --------------------------
    def _dev(self, t):
        if not (t.is_cuda and t.is_contiguous() and t.element_size() == 8):
            raise RingError("expected a contiguous CUDA tensor of 8-byte integers")
        if t.device.index != self.device:
            raise RingError("tensor lives on cuda:%d, this context on cuda:%d" % (t.device.index, self.device))
        return ctypes.c_void_p(t.data_ptr()), t.numel()

    def _stream(self, stream):
        import torch

        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        if s.device.index != self.device:
            raise RingError("stream belongs to cuda:%d, this context to cuda:%d" % (s.device.index, self.device))
        return ctypes.c_void_p(s.cuda_stream)

    # -- packed-u32 boundary (BabyBear power-of-two rings; include/stark_rings_hip.h "packed-u32 boundary") ------------------------
    # A packed tensor holds the LOW HALF of every reference limb: int32 / uint32 CUDA tensors of batch * D words, the uint32
    # (a * 2^64 mod p) of babybear/mod.rs:18-26's Fp64 -- same Montgomery residue, four bytes.
    def _dev32(self, t):
        if not (t.is_cuda and t.is_contiguous() and t.element_size() == 4):
            raise RingError("expected a contiguous CUDA tensor of 4-byte integers (packed-u32 image)")
        if t.device.index != self.device:
            raise RingError("tensor lives on cuda:%d, this context on cuda:%d" % (t.device.index, self.device))
        return ctypes.c_void_p(t.data_ptr()), t.numel()

    def pack32_dev(self, out32, in64, stream=None):
        """8-byte reference image -> packed image (low word of every limb; the input must be canonical)."""
        po, n = self._dev32(out32)
        pi, m = self._dev(in64)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_pack32_batch_dev(self._ctx, po, pi, self._batch_of(n), self._stream(stream)))
        return out32

    def unpack32_dev(self, out64, in32, stream=None):
        po, n = self._dev(out64)
        pi, m = self._dev32(in32)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_unpack32_batch_dev(self._ctx, po, pi, self._batch_of(n), self._stream(stream)))
        return out64

    def elementwise_crt_packed32_dev(self, t, stream=None):
        p, n = self._dev32(t)
        self._check(self._lib.sr_ntt_fwd_packed32_batch_dev(self._ctx, p, self._batch_of(n), self._stream(stream)))
        return t

    def elementwise_icrt_packed32_dev(self, t, stream=None):
        p, n = self._dev32(t)
        self._check(self._lib.sr_ntt_inv_packed32_batch_dev(self._ctx, p, self._batch_of(n), self._stream(stream)))
        return t

    def mul_packed32_dev(self, out, a, b, stream=None):
        """out = a * b on packed images (RqPoly * &RqPoly, coeff_form.rs:250-258); a and b are only read; out may be a."""
        po, n = self._dev32(out)
        pa, m = self._dev32(a)
        pb, q = self._dev32(b)
        if not (n == m == q):
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_ring_mul_packed32_batch_dev(self._ctx, po, pa, pb, self._batch_of(n), self._stream(stream)))
        return out

    def _ew32(self, fn, lhs, rhs, stream):
        pl, n = self._dev32(lhs)
        pr, m = self._dev32(rhs)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(fn(self._ctx, pl, pr, self._batch_of(n), self._stream(stream)))
        return lhs

    def ntt_mul_packed32_dev(self, lhs, rhs, stream=None):
        return self._ew32(self._lib.sr_pointwise_mul_packed32_batch_dev, lhs, rhs, stream)

    def add_packed32_dev(self, lhs, rhs, stream=None):
        return self._ew32(self._lib.sr_add_packed32_batch_dev, lhs, rhs, stream)

    def sub_packed32_dev(self, lhs, rhs, stream=None):
        return self._ew32(self._lib.sr_sub_packed32_batch_dev, lhs, rhs, stream)

    def reserve_scratch(self, batch):
        """sr_ctx_reserve_scratch: pre-size the operand scratch so that no later mul_dev of up to `batch` elements blocks.  With
        sr_plan.lanes = 0 (auto) this is also where the library times its two plans once and keeps the faster (plan_in_use)."""
        self._check(self._lib.sr_ctx_reserve_scratch(self._ctx, int(batch)))

    def plan_in_use(self):
        """sr_ctx_plan_in_use: (plan, probe) -- the context's sr_plan with `lanes` resolved to what the library settled on (0 = auto,
        not settled yet) and, when the library measured, {"two_lanes_ms", "one_stream_ms", "elems"} of its probe (else None)."""
        plan = _lib.Plan()
        ms = (ctypes.c_double * 2)()
        n = ctypes.c_size_t(0)
        self._check(self._lib.sr_ctx_plan_in_use(self._ctx, ctypes.byref(plan), ms, ctypes.byref(n)))
        probe = {"two_lanes_ms": ms[0], "one_stream_ms": ms[1], "elems": int(n.value)} if n.value else None
        return plan, probe

    def elementwise_crt_dev(self, t, stream=None):
        p, n = self._dev(t)
        self._check(self._lib.sr_ntt_fwd_batch_dev(self._ctx, p, self._batch_of(n), self._stream(stream)))
        return t

    def elementwise_icrt_dev(self, t, stream=None):
        p, n = self._dev(t)
        self._check(self._lib.sr_ntt_inv_batch_dev(self._ctx, p, self._batch_of(n), self._stream(stream)))
        return t

    def ntt_mul_dev(self, lhs, rhs, stream=None):
        pl, n = self._dev(lhs)
        pr, m = self._dev(rhs)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_pointwise_mul_batch_dev(self._ctx, pl, pr, self._batch_of(n), self._stream(stream)))
        return lhs

    def add_dev(self, lhs, rhs, stream=None):
        pl, n = self._dev(lhs)
        pr, m = self._dev(rhs)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_add_batch_dev(self._ctx, pl, pr, self._batch_of(n), self._stream(stream)))
        return lhs

    def sub_dev(self, lhs, rhs, stream=None):
        pl, n = self._dev(lhs)
        pr, m = self._dev(rhs)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_sub_batch_dev(self._ctx, pl, pr, self._batch_of(n), self._stream(stream)))
        return lhs

    def neg_dev(self, t, stream=None):
        p, n = self._dev(t)
        self._check(self._lib.sr_neg_batch_dev(self._ctx, p, self._batch_of(n), self._stream(stream)))
        return t

    def scale_dev(self, t, scalar, stream=None):
        p, n = self._dev(t)
        s = self._scalar(scalar)
        self._check(self._lib.sr_scale_batch_dev(self._ctx, p, _np_ptr(s), self._batch_of(n), self._stream(stream)))
        return t

    def mul_elem_dev(self, t, elem, stream=None):
        p, n = self._dev(t)
        pe, ne = self._dev(elem)
        if ne != self.words_per_elem:
            raise RingError("mul_elem: the multiplier is not one ring element")
        self._check(self._lib.sr_mul_elem_batch_dev(self._ctx, p, pe, self._batch_of(n), self._stream(stream)))
        return t

    def mul_elem_add_dev(self, acc, x, r, stream=None):
        """acc[e] += r * x[e] slot-wise (CRT/NTT form): AddAssign<(R, &Self)> of the dense MLE (crates/poly mle/dense.rs:288-317).
        r: one ring element outside acc and x; acc and x: the same tensor or disjoint."""
        pa, n = self._dev(acc)
        px, m = self._dev(x)
        pr, nr = self._dev(r)
        if n != m:
            raise RingError("operand lengths differ")
        if nr != self.words_per_elem:
            raise RingError("mul_elem_add: the multiplier is not one ring element")
        self._check(self._lib.sr_mul_elem_add_batch_dev(self._ctx, pa, px, pr, self._batch_of(n), self._stream(stream)))
        return acc

    def mle_plan(self, num_vars, n_fixed, order=MLE_LEADING):
        """sr_mle_plan: (work_elems, launches) of a fold of n_fixed of num_vars variables on this ring -- host arithmetic only."""
        work = ctypes.c_size_t()
        launches = ctypes.c_int()
        k = self.degree.bit_length() - 1 if self.ring <= STARK_POW2 else 0
        self._check(self._lib.sr_mle_plan(self.ring, k, int(num_vars), int(n_fixed), int(order), ctypes.byref(work), ctypes.byref(launches)))
        return work.value, launches.value

    def _mle_sizes(self, n_words, num_vars, point_words, out_words):
        n_evals = self._batch_of(n_words)
        n_fixed = self._batch_of(point_words)
        if num_vars < 0 or num_vars >= 48 or n_fixed > num_vars:
            raise RingError("mle_fix_variables: the point has more entries than the table has variables")
        if n_evals > 1 << num_vars:
            raise RingError("mle_fix_variables: more evaluations than 2^num_vars")
        if out_words != self.words_per_elem << (num_vars - n_fixed):
            raise RingError("mle_fix_variables: out must hold 2^(num_vars - n_fixed) elements")
        return n_evals, n_fixed

    def mle_fix_variables_dev(self, out, evals, num_vars, point, order=MLE_LEADING, work=None, stream=None):
        """sr_mle_fix_variables_dev: out = the table `evals` (n_evals <= 2^num_vars elements, the rest zero) with the variables of
        `point` fixed -- MLE_LEADING: DenseMultilinearExtension::fix_variables (mle/dense.rs:171-199); MLE_TRAILING:
        fix_last_variables (multilinear_polynomial.rs:227-286), where out may be evals.  work: a tensor of at least mle_plan()[0]
        elements (None only where the plan needs none)."""
        po, no = self._dev(out)
        n_ev = evals.numel()
        pp, npt = (self._dev(point) if point is not None and point.numel() else (ctypes.c_void_p(0), 0))
        n_evals, n_fixed = self._mle_sizes(n_ev, num_vars, npt, no)
        pe = self._dev(evals)[0] if n_ev else ctypes.c_void_p(0)
        if work is None:
            pw, nw = ctypes.c_void_p(0), 0
        else:
            pw, nw = self._dev(work)
            nw //= self.words_per_elem
        self._check(self._lib.sr_mle_fix_variables_dev(self._ctx, po, pe, n_evals, int(num_vars), pp, n_fixed, int(order), pw, nw,
                                                       self._stream(stream)))
        return out

    def prod_tree_plan(self, num_vars, order=MLE_TRAILING):
        """sr_prod_tree_plan: (layer_elems, launches) of the product tree over 2^num_vars leaves on this ring -- host arithmetic only."""
        elems = ctypes.c_size_t()
        launches = ctypes.c_int()
        k = self.degree.bit_length() - 1 if self.ring <= STARK_POW2 else 0
        self._check(self._lib.sr_prod_tree_plan(self.ring, k, int(num_vars), int(order), ctypes.byref(elems), ctypes.byref(launches)))
        return elems.value, launches.value

    def _prod_tree_sizes(self, leaf_words, num_vars, layer_words):
        n_leaves = self._batch_of(leaf_words)
        if num_vars < 0 or num_vars >= 48:
            raise RingError("prod_tree: num_vars must be in [0, 48)")
        if n_leaves > 1 << num_vars:
            raise RingError("prod_tree: more leaves than 2^num_vars")
        if layer_words != self.words_per_elem * ((1 << num_vars) - 1):
            raise RingError("prod_tree: layers must hold 2^num_vars - 1 elements")
        return n_leaves

    def prod_tree_dev(self, layers, leaves, num_vars, order=MLE_TRAILING, stream=None):
        """sr_prod_tree_dev: every layer of the product tree over `leaves` (n_leaves <= 2^num_vars elements in CRT/NTT form, the rest
        one() and never read) into `layers` (2^num_vars - 1 elements: layer k at element offset 2^num_vars - 2^(num_vars - k + 1), the
        root last).  MLE_LEADING pairs (2i, 2i + 1), MLE_TRAILING pairs (i, i + half).  Allocates nothing."""
        null = ctypes.c_void_p(0)
        n_words = leaves.numel() if leaves is not None else 0
        n_leaves = self._prod_tree_sizes(n_words, num_vars, layers.numel())
        pl = self._dev(layers)[0] if layers.numel() else null
        pe = self._dev(leaves)[0] if n_words else null
        self._check(self._lib.sr_prod_tree_dev(self._ctx, pl, pe, n_leaves, int(num_vars), int(order), self._stream(stream)))
        return layers

    def prod_tree(self, leaves, num_vars, order=MLE_TRAILING):
        """Host buffers: sr_prod_tree (see prod_tree_dev); returns the 2^num_vars - 1 elements of the layers."""
        leaves = np.ascontiguousarray(leaves, dtype=np.uint64)
        n_out = self.words_per_elem * ((1 << num_vars) - 1) if 0 <= num_vars < 48 else 0
        n_leaves = self._prod_tree_sizes(leaves.size, num_vars, n_out)
        out = np.empty(max(n_out, 1), dtype=np.uint64)
        z = np.zeros(1, dtype=np.uint64)
        self._check(self._lib.sr_prod_tree(self._ctx, _np_ptr(out), _np_ptr(leaves if n_leaves else z), n_leaves, int(num_vars), int(order)))
        return out[:n_out]

    # ---- sum-check round messages: seven families (range_check.py holds the seventh), one set of argument helpers ----
    def _plan_of(self, fn, num_vars, n_tables, *shape):
        """(work_elems, launches) of a round family's *_plan call; shape: what the call takes after n_tables (n_terms and degree, or
        the bound; then the mode or order)"""
        work = ctypes.c_size_t()
        launches = ctypes.c_int()
        k = self.degree.bit_length() - 1 if self.ring <= STARK_POW2 else 0
        self._check(fn(self.ring, k, int(num_vars), int(n_tables), *[int(s) for s in shape], ctypes.byref(work), ctypes.byref(launches)))
        return work.value, launches.value

    def _round_dev_args(self, what, out, out_elems, out_text, tables, work, coeffs=None, n_coeffs=0, per="term", weights=None, pairs_log2=-1):
        """the arguments the round-message device calls share: (po, ptrs, sizes, n, pc, pweights, pwork, nwork).  out_elems: what out
        must hold (None: the library decides), out_text: how the error says it; coeffs: n_coeffs elements, one per `per`, or None;
        weights: 2^pairs_log2 elements or None"""
        null = ctypes.c_void_p(0)
        po, no = self._dev(out)
        n = len(tables)
        if out_elems is not None and no != self.words_per_elem * out_elems:
            raise RingError(what + ": out must hold " + out_text)
        pwt = null
        if weights is not None:
            pwt, nwt = self._dev(weights)
            if 0 <= pairs_log2 < 48 and nwt != self.words_per_elem << pairs_log2:
                raise RingError(what + ": weights must hold one element per pair (2^%d)" % pairs_log2)
        ptrs = (ctypes.c_void_p * max(n, 1))()
        sizes = (ctypes.c_size_t * max(n, 1))()
        for j, t in enumerate(tables):
            sizes[j] = self._batch_of(t.numel())
            ptrs[j] = self._dev(t)[0] if t.numel() else None
        pc = null
        if coeffs is not None:
            pc, nc = self._dev(coeffs)
            if nc != n_coeffs * self.words_per_elem:
                raise RingError(what + ": one coefficient per " + per)
        pw, nw = null, 0
        if work is not None:
            pw, nw = self._dev(work)
            nw //= self.words_per_elem
        return po, ptrs, sizes, n, pc, pwt, pw, nw

    def _fold_dev_args(self, what, out_tables, sizes, n, num_vars, r, order):
        """what a fold's device call takes besides: (optrs, osizes, pr)"""
        if len(out_tables) != n:
            raise RingError(what + ": one output table per table")
        pr, nr = self._dev(r)
        if nr != self.words_per_elem:
            raise RingError(what + ": r is not one ring element")
        optrs = (ctypes.c_void_p * max(n, 1))()
        osizes = (ctypes.c_size_t * max(n, 1))()
        for j, o in enumerate(out_tables):
            optrs[j] = self._dev(o)[0] if o.numel() else None
            if 2 <= num_vars < 48:
                need = (sizes[j] + 1) // 2 if order == MLE_LEADING else min(sizes[j], 1 << (num_vars - 1))
                if o.numel() < need * self.words_per_elem:
                    raise RingError(what + ": an output table is shorter than the folded table")
        return optrs, osizes, pr

    def _round_host_args(self, what, out_elems, tables, coeffs=None, n_coeffs=0, per="term", weights=None):
        """the arguments the host-pointer round calls share: (tables, weights, coeffs, out, ptrs, sizes, n); the arrays are returned so
        that they outlive the call"""
        tables = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
        weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
        n = len(tables)
        out = np.empty(self.words_per_elem * out_elems, dtype=np.uint64)
        ptrs = (ctypes.c_void_p * max(n, 1))()
        sizes = (ctypes.c_size_t * max(n, 1))()
        for j, t in enumerate(tables):
            sizes[j] = self._batch_of(t.size)
            ptrs[j] = t.ctypes.data if t.size else None
        if coeffs is not None:
            coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64)
            if coeffs.size != n_coeffs * self.words_per_elem:
                raise RingError(what + ": one coefficient per " + per)
        return tables, weights, coeffs, out, ptrs, sizes, n

    def _fold_host_args(self, what, tables, r):
        """what a fold's host-pointer call takes besides: (r, folded, optrs, osizes); tables: the arrays of _round_host_args"""
        r = np.ascontiguousarray(r, dtype=np.uint64)
        if r.size != self.words_per_elem:
            raise RingError(what + ": r is not one ring element")
        n = len(tables)
        optrs = (ctypes.c_void_p * max(n, 1))()
        osizes = (ctypes.c_size_t * max(n, 1))()
        folded = [np.empty(t.size, dtype=np.uint64) for t in tables]  # never shorter than the folded table
        for j, t in enumerate(tables):
            optrs[j] = folded[j].ctypes.data if t.size else None
        return r, folded, optrs, osizes

    def mle_round_plan(self, num_vars, n_tables, mode=MLE_LEADING):
        """sr_mle_round_plan: (work_elems, launches) of a sum-check round message over n_tables tables -- host arithmetic only."""
        return self._plan_of(self._lib.sr_mle_round_plan, num_vars, n_tables, mode)

    def mle_round_evals_dev(self, out, tables, num_vars, mode=MLE_LEADING, work=None, stream=None):
        """sr_mle_round_evals_dev: the prover's message of a sum-check round over the product of `tables` (1 .. 4 CUDA tensors, each
        n_evals <= 2^num_vars elements, the rest zero; a table may appear twice).  MLE_LEADING / MLE_TRAILING: out[t] = sum over the
        pairs of prod_j (lo_j + t (hi_j - lo_j)) for t = 0 .. len(tables), the pair being (f[2b], f[2b+1]) or (f[b], f[b + half]);
        MLE_ROUND_SUM: out = sum_b prod_j f_j[b], one element.  work: a tensor of at least mle_round_plan()[0] elements (None only
        where the plan needs none).  Allocates nothing."""
        po, ptrs, sizes, n, _, _, pw, nw = self._round_dev_args("mle_round_evals", out, 1 if mode == MLE_ROUND_SUM else len(tables) + 1,
                                                                "len(tables) + 1 elements (one for MLE_ROUND_SUM)", tables, work)
        self._check(self._lib.sr_mle_round_evals_dev(self._ctx, po, ptrs, sizes, n, int(num_vars), int(mode), pw, nw, self._stream(stream)))
        return out

    def mle_round_evals(self, tables, num_vars, mode=MLE_LEADING):
        """Host buffers: sr_mle_round_evals (see mle_round_evals_dev); returns the len(tables) + 1 elements (one for MLE_ROUND_SUM)."""
        tables, _, _, out, ptrs, sizes, n = self._round_host_args("mle_round_evals", 1 if mode == MLE_ROUND_SUM else len(tables) + 1, tables)
        self._check(self._lib.sr_mle_round_evals(self._ctx, _np_ptr(out), ptrs, sizes, n, int(num_vars), int(mode)))
        return out

    @staticmethod
    def _vpoly_terms(terms):
        """a list of index lists -> (the sr_vpoly_term array, n_terms, the largest factor count); the library checks the limits"""
        from ._lib import VPOLY_MAX_FACTORS, VPolyTerm
        arr = (VPolyTerm * max(len(terms), 1))()
        for k, t in enumerate(terms):
            t = list(t)
            arr[k].n_factors = len(t)
            for s, j in enumerate(t[:VPOLY_MAX_FACTORS]):
                arr[k].table[s] = int(j)
        return arr, len(terms), max([len(list(t)) for t in terms] or [0])

    def vpoly_round_plan(self, num_vars, n_tables, n_terms, degree, mode=MLE_LEADING):
        """sr_vpoly_round_plan: (work_elems, launches) of a round message over a sum of n_terms products of at most `degree` of
        n_tables tables -- host arithmetic only."""
        return self._plan_of(self._lib.sr_vpoly_round_plan, num_vars, n_tables, n_terms, degree, mode)

    def vpoly_round_evals_dev(self, out, tables, terms, coeffs, num_vars, mode=MLE_LEADING, work=None, stream=None):
        """sr_vpoly_round_evals_dev: the prover's message of a sum-check round over g = sum_k c_k prod_s f_{terms[k][s]} in one pass
        that reads every table once.  tables: 1 .. 8 CUDA tensors (n_evals <= 2^num_vars elements each, the rest zero); terms: 1 .. 8
        lists of 1 .. 4 indices into `tables`; coeffs: a CUDA tensor of len(terms) ring elements, or None for one() everywhere.
        MLE_LEADING / MLE_TRAILING: out[t] for t = 0 .. d, d the longest term; MLE_ROUND_SUM: out = sum_b g(b), one element.  work: a
        tensor of at least vpoly_round_plan()[0] elements (None only where the plan needs none).  Allocates nothing."""
        arr, n_terms, d = self._vpoly_terms(terms)
        po, ptrs, sizes, n, pc, _, pw, nw = self._round_dev_args("vpoly_round_evals", out, 1 if mode == MLE_ROUND_SUM else d + 1,
                                                                 "d + 1 elements, d the longest term (one for MLE_ROUND_SUM)", tables, work,
                                                                 coeffs, n_terms)
        self._check(self._lib.sr_vpoly_round_evals_dev(self._ctx, po, ptrs, sizes, n, arr, n_terms, pc, int(num_vars), int(mode), pw, nw,
                                                       self._stream(stream)))
        return out

    def vpoly_round_evals(self, tables, terms, coeffs, num_vars, mode=MLE_LEADING):
        """Host buffers: sr_vpoly_round_evals (see vpoly_round_evals_dev); returns the d + 1 elements (one for MLE_ROUND_SUM)."""
        arr, n_terms, d = self._vpoly_terms(terms)
        tables, _, coeffs, out, ptrs, sizes, n = self._round_host_args("vpoly_round_evals", 1 if mode == MLE_ROUND_SUM else max(d, 1) + 1,
                                                                       tables, coeffs, n_terms)
        self._check(self._lib.sr_vpoly_round_evals(self._ctx, _np_ptr(out), ptrs, sizes, n, arr, n_terms,
                                                   None if coeffs is None else coeffs.ctypes.data, int(num_vars), int(mode)))
        return out

    def mle_round_fold_plan(self, num_vars, n_tables, order=MLE_LEADING):
        """sr_mle_round_fold_plan: (work_elems, launches) of the fused fold-and-round call over n_tables tables of num_vars >= 2
        variables -- host arithmetic only."""
        return self._plan_of(self._lib.sr_mle_round_fold_plan, num_vars, n_tables, order)

    def mle_round_fold_evals_dev(self, out, out_tables, tables, num_vars, r, order=MLE_LEADING, work=None, stream=None):
        """sr_mle_round_fold_evals_dev: one pass that folds every table of `tables` (1 .. 4 CUDA tensors of n_evals <= 2^num_vars
        elements, num_vars >= 2) at the ring element `r` into out_tables[j] -- what mle_fix_variables_dev gives for one variable, in
        truncated storage -- and writes to out[t], t = 0 .. len(tables), the message of the next round over the folded tables
        (mle_round_evals_dev on them).  out_tables[j] must hold at least the folded length; MLE_TRAILING may fold in place
        (out_tables[j] is tables[j]).  Returns the list of elements written per table; nothing beyond them is touched.  work: a tensor
        of at least mle_round_fold_plan()[0] elements (None only where the plan needs none).  Allocates nothing."""
        what = "mle_round_fold_evals"
        po, ptrs, sizes, n, _, _, pw, nw = self._round_dev_args(what, out, len(tables) + 1, "len(tables) + 1 elements", tables, work)
        optrs, osizes, pr = self._fold_dev_args(what, out_tables, sizes, n, num_vars, r, order)
        self._check(self._lib.sr_mle_round_fold_evals_dev(self._ctx, po, optrs, osizes, ptrs, sizes, n, int(num_vars), pr, int(order), pw, nw,
                                                          self._stream(stream)))
        return [int(osizes[j]) for j in range(n)]

    def mle_round_fold_evals(self, tables, num_vars, r, order=MLE_LEADING):
        """Host buffers: sr_mle_round_fold_evals (see mle_round_fold_evals_dev); returns (message, list of folded tables)."""
        what, w = "mle_round_fold_evals", self.words_per_elem
        tables, _, _, out, ptrs, sizes, n = self._round_host_args(what, len(tables) + 1, tables)
        r, folded, optrs, osizes = self._fold_host_args(what, tables, r)
        self._check(self._lib.sr_mle_round_fold_evals(self._ctx, _np_ptr(out), optrs, osizes, ptrs, sizes, n, int(num_vars), _np_ptr(r),
                                                      int(order)))
        return out, [f[:int(osizes[j]) * w] for j, f in enumerate(folded)]

    def vpoly_round_fold_plan(self, num_vars, n_tables, n_terms, degree, order=MLE_LEADING):
        """sr_vpoly_round_fold_plan: (work_elems, launches) of the fused fold-and-round call over a sum of n_terms products of at
        most `degree` of n_tables tables of num_vars >= 2 variables -- host arithmetic only."""
        return self._plan_of(self._lib.sr_vpoly_round_fold_plan, num_vars, n_tables, n_terms, degree, order)

    def vpoly_round_fold_evals_dev(self, out, out_tables, tables, terms, coeffs, num_vars, r, order=MLE_LEADING, work=None, stream=None):
        """sr_vpoly_round_fold_evals_dev: one pass that folds every table slot of `tables` (1 .. 8 CUDA tensors of n_evals <=
        2^num_vars elements, num_vars >= 2) at the ring element `r` into out_tables[j] -- what mle_fix_variables_dev gives for one
        variable, in truncated storage -- and writes to out[t], t = 0 .. d (d the longest term), the message of the next round of
        g = sum_k c_k prod_s f_{terms[k][s]} over the folded tables (vpoly_round_evals_dev on them).  terms, coeffs: as in
        vpoly_round_evals_dev.  out_tables[j] must hold at least the folded length; MLE_TRAILING may fold in place (out_tables[j] is
        tables[j]).  Returns the list of elements written per table; nothing beyond them is touched.  work: a tensor of at least
        vpoly_round_fold_plan()[0] elements (None only where the plan needs none).  Allocates nothing."""
        what = "vpoly_round_fold_evals"
        arr, n_terms, d = self._vpoly_terms(terms)
        po, ptrs, sizes, n, pc, _, pw, nw = self._round_dev_args(what, out, d + 1, "d + 1 elements, d the longest term", tables, work, coeffs,
                                                                 n_terms)
        optrs, osizes, pr = self._fold_dev_args(what, out_tables, sizes, n, num_vars, r, order)
        self._check(self._lib.sr_vpoly_round_fold_evals_dev(self._ctx, po, optrs, osizes, ptrs, sizes, n, arr, n_terms, pc, int(num_vars), pr,
                                                            int(order), pw, nw, self._stream(stream)))
        return [int(osizes[j]) for j in range(n)]

    def vpoly_round_fold_evals(self, tables, terms, coeffs, num_vars, r, order=MLE_LEADING):
        """Host buffers: sr_vpoly_round_fold_evals (see vpoly_round_fold_evals_dev); returns (message, list of folded tables)."""
        what, w = "vpoly_round_fold_evals", self.words_per_elem
        arr, n_terms, d = self._vpoly_terms(terms)
        tables, _, coeffs, out, ptrs, sizes, n = self._round_host_args(what, max(d, 1) + 1, tables, coeffs, n_terms)
        r, folded, optrs, osizes = self._fold_host_args(what, tables, r)
        self._check(self._lib.sr_vpoly_round_fold_evals(self._ctx, _np_ptr(out), optrs, osizes, ptrs, sizes, n, arr, n_terms,
                                                        None if coeffs is None else coeffs.ctypes.data, int(num_vars), _np_ptr(r), int(order)))
        return out, [f[:int(osizes[j]) * w] for j, f in enumerate(folded)]

    def vpoly_wround_plan(self, num_vars, n_tables, n_terms, degree, order=MLE_LEADING):
        """sr_vpoly_wround_plan: (work_elems, launches) of a weighted round message (vpoly_wround_evals_dev) -- host arithmetic only."""
        return self._plan_of(self._lib.sr_vpoly_wround_plan, num_vars, n_tables, n_terms, degree, order)

    def vpoly_wround_fold_plan(self, num_vars, n_tables, n_terms, degree, order=MLE_LEADING):
        """sr_vpoly_wround_fold_plan: (work_elems, launches) of the weighted fused fold-and-round call (vpoly_wround_fold_evals_dev),
        num_vars >= 2 -- host arithmetic only."""
        return self._plan_of(self._lib.sr_vpoly_wround_fold_plan, num_vars, n_tables, n_terms, degree, order)

    def _vpoly_wround_evals_dev(self, out, weights, tables, terms, coeffs, num_vars, order=MLE_LEADING, work=None, stream=None):
        """sr_vpoly_wround_evals_dev (public as stark_rings_amd.wsumcheck.vpoly_wround_evals_dev): the round message of
        vpoly_round_evals_dev with a per-pair weight,
        out[t] = sum_{b < half} weights[b] * sum_k c_k prod_s (lo_s[b] + t (hi_s[b] - lo_s[b])), t = 0 .. d (d the longest term; the
        weight is not a factor).  weights: a CUDA tensor of 2^(num_vars - 1) ring elements, one per pair, never written; order:
        MLE_LEADING or MLE_TRAILING.  The rest as vpoly_round_evals_dev.  work: at least vpoly_wround_plan()[0] elements."""
        arr, n_terms, d = self._vpoly_terms(terms)
        po, ptrs, sizes, n, pc, pwt, pw, nw = self._round_dev_args("vpoly_wround_evals", out, d + 1, "d + 1 elements, d the longest term", tables,
                                                                   work, coeffs, n_terms, "term", weights, num_vars - 1)
        self._check(self._lib.sr_vpoly_wround_evals_dev(self._ctx, po, pwt, ptrs, sizes, n, arr, n_terms, pc, int(num_vars), int(order), pw, nw,
                                                        self._stream(stream)))
        return out

    def _vpoly_wround_fold_evals_dev(self, out, out_tables, weights, tables, terms, coeffs, num_vars, r, order=MLE_LEADING, work=None,
                                    stream=None):
        """sr_vpoly_wround_fold_evals_dev (public as stark_rings_amd.wsumcheck.vpoly_wround_fold_evals_dev): vpoly_round_fold_evals_dev
        with a per-pair weight on the message: the tables are folded at
        `r` into out_tables exactly as there, and out[t], t = 0 .. d, is vpoly_wround_evals_dev on the folded tables at num_vars - 1
        with the same `weights` (2^(num_vars - 2) ring elements).  Returns the list of elements written per table.  work: at least
        vpoly_wround_fold_plan()[0] elements."""
        what = "vpoly_wround_fold_evals"
        arr, n_terms, d = self._vpoly_terms(terms)
        po, ptrs, sizes, n, pc, pwt, pw, nw = self._round_dev_args(what, out, d + 1, "d + 1 elements, d the longest term", tables, work, coeffs,
                                                                   n_terms, "term", weights, num_vars - 2)
        optrs, osizes, pr = self._fold_dev_args(what, out_tables, sizes, n, num_vars, r, order)
        self._check(self._lib.sr_vpoly_wround_fold_evals_dev(self._ctx, po, optrs, osizes, pwt, ptrs, sizes, n, arr, n_terms, pc, int(num_vars),
                                                             pr, int(order), pw, nw, self._stream(stream)))
        return [int(osizes[j]) for j in range(n)]

    def vpoly_wround_evals(self, weights, tables, terms, coeffs, num_vars, order=MLE_LEADING):
        """Host buffers: sr_vpoly_wround_evals (see vpoly_wround_evals_dev); returns the d + 1 elements."""
        arr, n_terms, d = self._vpoly_terms(terms)
        tables, weights, coeffs, out, ptrs, sizes, n = self._round_host_args("vpoly_wround_evals", max(d, 1) + 1, tables, coeffs, n_terms, "term",
                                                                             weights)
        if weights is not None and 1 <= num_vars < 48 and weights.size != self.words_per_elem << (num_vars - 1):
            raise RingError("vpoly_wround_evals: weights must hold one element per pair")
        self._check(self._lib.sr_vpoly_wround_evals(self._ctx, _np_ptr(out), None if weights is None else weights.ctypes.data, ptrs, sizes, n, arr,
                                                    n_terms, None if coeffs is None else coeffs.ctypes.data, int(num_vars), int(order)))
        return out

    def vpoly_wround_fold_evals(self, weights, tables, terms, coeffs, num_vars, r, order=MLE_LEADING):
        """Host buffers: sr_vpoly_wround_fold_evals (see vpoly_wround_fold_evals_dev); returns (message, list of folded tables)."""
        what, w = "vpoly_wround_fold_evals", self.words_per_elem
        arr, n_terms, d = self._vpoly_terms(terms)
        tables, weights, coeffs, out, ptrs, sizes, n = self._round_host_args(what, max(d, 1) + 1, tables, coeffs, n_terms, "term", weights)
        r, folded, optrs, osizes = self._fold_host_args(what, tables, r)
        if weights is not None and 2 <= num_vars < 48 and weights.size != w << (num_vars - 2):
            raise RingError("vpoly_wround_fold_evals: weights must hold one element per pair of the folded tables")
        self._check(self._lib.sr_vpoly_wround_fold_evals(self._ctx, _np_ptr(out), optrs, osizes, None if weights is None else weights.ctypes.data,
                                                         ptrs, sizes, n, arr, n_terms, None if coeffs is None else coeffs.ctypes.data,
                                                         int(num_vars), _np_ptr(r), int(order)))
        return out, [f[:int(osizes[j]) * w] for j, f in enumerate(folded)]

    def eq_table_dev(self, out, point, stream=None):
        """sr_eq_table_dev: out[b] = prod_i (bit i of b ? point[i] : 1 - point[i]) for the n = len(point) elements of `point`
        (None or empty: out is the single element one()); out holds 2^n elements.  One launch, no workspace; capturable."""
        po, no = self._dev(out)
        pp, npt = (self._dev(point) if point is not None and point.numel() else (ctypes.c_void_p(0), 0))
        n = self._batch_of(npt)
        if n >= 48 or no != self.words_per_elem << n:
            raise RingError("eq_table: out must hold 2^len(point) elements")
        self._check(self._lib.sr_eq_table_dev(self._ctx, po, pp, n, self._stream(stream)))
        return out

    def smle_plan(self, nnz, n_out, n_fixed):
        """sr_smle_plan for this ring: (work_elems, launches)."""
        return smle_plan(self.ring, self.degree.bit_length() - 1 if self.ring <= STARK_POW2 else 0, nnz, n_out, n_fixed)

    smle_fix_pattern = staticmethod(smle_fix_pattern)

    def smle_fix_variables_dev(self, out_vals, vals, idx, seg_ptr, point, work=None, stream=None):
        """sr_smle_fix_variables_dev: out_vals[s] = sum over run s of eq(point, idx[j] & (2^n_fixed - 1)) * vals[j].  idx (nnz) and
        seg_ptr (n_out + 1) are int64 / uint64 CUDA tensors holding what smle_fix_pattern saw and returned; out_vals holds n_out
        elements.  work: a tensor of at least smle_plan()[0] elements (None only where the plan needs none).  Allocates nothing."""
        nnz = idx.numel()
        n_out = seg_ptr.numel() - 1
        if n_out < 0 or self._batch_of(vals.numel()) != nnz or self._batch_of(out_vals.numel()) != n_out:
            raise RingError("smle_fix_variables: one value per index and one output element per run")
        null = ctypes.c_void_p(0)
        pp, npt = (self._dev(point) if point is not None and point.numel() else (null, 0))
        pw, nw = (self._dev(work) if work is not None and work.numel() else (null, 0))
        self._check(self._lib.sr_smle_fix_variables_dev(self._ctx, self._dev(out_vals)[0] if n_out else null, self._dev(vals)[0] if nnz else null,
                                                        self._dev(idx)[0] if nnz else null, nnz, self._dev(seg_ptr)[0], n_out, pp,
                                                        self._batch_of(npt), pw, nw // self.words_per_elem, self._stream(stream)))
        return out_vals

    def norm_batch_dev(self, out, coeffs, group=None, which=NORM_LINF | NORM_L2SQ, work=None, stream=None):
        """sr_norm_batch_dev: out = the records (norm_plan()[0] words per group: linf words, then l2sq words; standard-form integers)
        of the device-resident coefficients.  work: a tensor of at least norm_plan()[1] words (None only where the plan needs none).
        Allocates nothing; capturable."""
        po, no = self._dev(out)
        n = self._norm_coeffs(coeffs.numel())
        g = self._norm_group(n, group)
        if g and n % g == 0 and no != max(n // g, 1) * self.norm_plan(n, g, which)[0]:
            raise RingError("norm: out must hold norm_plan()[0] words per group")
        pc = self._dev(coeffs)[0] if n else ctypes.c_void_p(0)
        pw, nw = self._dev(work) if work is not None else (ctypes.c_void_p(0), 0)
        self._check(self._lib.sr_norm_batch_dev(self._ctx, po, pc, n, g, int(which), pw, nw, self._stream(stream)))
        return out

    def _norm_dev(self, coeffs, group, which, work, stream):
        import torch

        n = self._norm_coeffs(coeffs.numel())
        g = self._norm_group(n, group)
        wpg, need, _ = self.norm_plan(n, g, which)
        out = torch.empty(max(n // g, 1) * wpg, dtype=torch.int64, device=coeffs.device)
        if work is None and need:
            work = torch.empty(need, dtype=torch.int64, device=coeffs.device)
        self.norm_batch_dev(out, coeffs, g, which, work, stream)
        return self._norm_ints(out.cpu().numpy().view(np.uint64), which, group is None)  # the copy synchronises

    def linf_norm_dev(self, coeffs, group=None, work=None, stream=None):
        """linf_norm of a device tensor of coefficients, as Python int(s); work: an optional caller workspace (norm_plan()[1] words)."""
        return self._norm_dev(coeffs, group, NORM_LINF, work, stream)

    def l2_norm_squared_dev(self, coeffs, group=None, work=None, stream=None):
        return self._norm_dev(coeffs, group, NORM_L2SQ, work, stream)

    def norms_dev(self, coeffs, group=None, work=None, stream=None):
        """(linf, l2sq) of a device tensor from one pass (see norms)."""
        return self._norm_dev(coeffs, group, NORM_LINF | NORM_L2SQ, work, stream)

    def sum_dev(self, out, elems, stream=None):
        """Sum over a device-resident slice (see sum): out = one ring element, must not overlap elems."""
        if out.numel() != self.words_per_elem:
            raise RingError("sum: out is not one ring element")
        n = self._batch_of(elems.numel())
        po = self._dev(out)[0]
        self._check(self._lib.sr_sum_batch_dev(self._ctx, po, self._dev(elems)[0] if n else po, n, self._stream(stream)))
        return out

    def product_dev(self, out, elems_ntt, stream=None):
        """Product over a device-resident slice in CRT/NTT form (see product)."""
        if out.numel() != self.words_per_elem:
            raise RingError("product: out is not one ring element")
        n = self._batch_of(elems_ntt.numel())
        po = self._dev(out)[0]
        self._check(self._lib.sr_product_batch_dev(self._ctx, po, self._dev(elems_ntt)[0] if n else po, n, self._stream(stream)))
        return out

    def product_poly_dev(self, out, elems, stream=None):
        """Product of coefficient-form elements (see product_poly); `elems` is transformed IN PLACE (it holds crt(elems) afterwards)."""
        if elems.numel():
            self.elementwise_crt_dev(elems, stream=stream)
        self.product_dev(out, elems, stream=stream)
        return self.elementwise_icrt_dev(out, stream=stream)

    def add_scalar_dev(self, t, scalar, ntt_form, stream=None):
        p, n = self._dev(t)
        s = self._scalar(scalar)
        self._check(self._lib.sr_add_scalar_batch_dev(self._ctx, p, _np_ptr(s), 1 if ntt_form else 0, self._batch_of(n), self._stream(stream)))
        return t

    def matvec_ntt_dev(self, y, m, v, nrows, ncols, stream=None):
        """y = M v for M (nrows x ncols ring elements, row-major) and v (ncols elements), all in CRT/NTT form:
        Matrix<RqNTT>::checked_mul_vec (linear_algebra/src/matrix.rs:168-178); the reference returns None on a length
        mismatch, here RingError is raised."""
        py, ny = self._dev(y)
        pm, nm = self._dev(m)
        pv, nv = self._dev(v)
        if nm != nrows * ncols * self.words_per_elem or nv != ncols * self.words_per_elem or ny != nrows * self.words_per_elem:
            raise RingError("matvec: DifferentLengths")
        self._check(self._lib.sr_matvec_ntt_dev(self._ctx, py, pm, pv, nrows, ncols, self._stream(stream)))
        return y

    def spmv_ntt_dev(self, y, vals, cols, row_ptr, v, nrows, ncols, stream=None):
        """y = S v for a CSR sparse matrix of ring elements in CRT/NTT form: SparseMatrix<RqNTT>::checked_mul_vec
        (linear_algebra/src/sparse_matrix.rs:201-211).  vals: nnz ring elements (int64 words), cols: int32 column of each,
        row_ptr: int64 [nrows + 1].  Entries whose column is >= ncols are skipped and counted (spmv_bad_index_count)."""
        import torch

        py, ny = self._dev(y)
        pv, nv = self._dev(v)
        if cols.dtype != torch.int32 or row_ptr.dtype != torch.int64 or row_ptr.numel() != nrows + 1:
            raise RingError("spmv: cols must be int32 and row_ptr int64 of length nrows + 1")
        nnz = cols.numel()
        if vals.numel() != nnz * self.words_per_elem or nv != ncols * self.words_per_elem or ny != nrows * self.words_per_elem:
            raise RingError("spmv: DifferentLengths")
        pvals = self._dev(vals)[0] if nnz else 0
        self._check(self._lib.sr_spmv_ntt_dev(self._ctx, py, pvals, cols.data_ptr() if nnz else 0, row_ptr.data_ptr(), pv,
                                              nrows, ncols, self._stream(stream)))
        return y

    def spmv_bad_index_count(self, stream=None):
        import ctypes

        n = ctypes.c_ulonglong(0)
        self._check(self._lib.sr_spmv_bad_index_count(self._ctx, ctypes.byref(n), self._stream(stream)))
        return int(n.value)

    def matmul_ntt_dev(self, y, a, b, n, m, p, stream=None):
        """Y (n x p) = A (n x m) B (m x p), dense row-major, CRT/NTT form: Matrix<RqNTT>::checked_mul_mat
        (linear_algebra/src/matrix.rs:148-166)."""
        py, ny = self._dev(y)
        pa, na = self._dev(a)
        pb, nb = self._dev(b)
        w = self.words_per_elem
        if na != n * m * w or nb != m * p * w or ny != n * p * w:
            raise RingError("matmul: DifferentLengths")
        self._check(self._lib.sr_matmul_ntt_dev(self._ctx, py, pa, pb, n, m, p, self._stream(stream)))
        return y

    def gram_plan(self, n, m):
        """sr_gram_plan for this ring: (work_elems, launches)."""
        return gram_plan(self.ring, self.degree.bit_length() - 1, n, m)

    def symm_recompose_plan(self, n, d):
        """sr_symm_recompose_plan for this ring: (work_elems, launches)."""
        return symm_recompose_plan(self.ring, self.degree.bit_length() - 1, n, d)

    def _dev_or_null(self, t):
        return self._dev(t) if t is not None and t.numel() else (ctypes.c_void_p(0), 0)

    def gram_ntt_dev(self, out, a, n, m, work=None, stream=None):
        """sr_gram_ntt_dev: out (packed, n (n + 1) / 2 elements) = the Gram matrix of the rows of the dense n x m matrix a.  work: a
        tensor of at least gram_plan()[0] elements (None where the plan needs none).  Allocates nothing; capturable."""
        w = self.words_per_elem
        po, no = self._dev_or_null(out)
        pa, na = self._dev_or_null(a)
        pw, nw = self._dev_or_null(work)
        if n < 0 or m < 0 or na != n * m * w or no != n * (n + 1) // 2 * w:
            raise RingError("gram: DifferentLengths")
        self._check(self._lib.sr_gram_ntt_dev(self._ctx, po, pa, n, m, pw, nw // w, self._stream(stream)))
        return out

    def symm_recompose_dev(self, out, mat, n, d, powers, work, stream=None):
        """sr_symm_recompose_dev: out (packed, size n) = G^T mat G for the packed matrix mat of size n * d and the d elements
        `powers`.  work: a tensor of at least symm_recompose_plan()[0] elements.  Allocates nothing; capturable."""
        w = self.words_per_elem
        po, no = self._dev_or_null(out)
        pm, nm = self._dev_or_null(mat)
        pp, npw = self._dev_or_null(powers)
        pw, nw = self._dev_or_null(work)
        if n < 0 or d < 0 or npw != d * w or nm != (n * d) * (n * d + 1) // 2 * w or no != n * (n + 1) // 2 * w:
            raise RingError("symm_recompose: DifferentLengths")
        self._check(self._lib.sr_symm_recompose_dev(self._ctx, po, pm, n, d, pp, pw, nw // w, self._stream(stream)))
        return out

    def spgemm_plan(self, n_out, n_pairs):
        """sr_spgemm_plan for this ring: (work_elems, launches)."""
        return spgemm_plan(self.ring, self.degree.bit_length() - 1, n_out, n_pairs)

    def _dev_idx(self, t, dtype, what):
        """(pointer, length) of an index tensor on this context's device; None or empty: (null, 0)"""
        if t is None or t.numel() == 0:
            return ctypes.c_void_p(0), 0
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype and t.device.index == self.device):
            raise RingError("%s must be a contiguous %s tensor on cuda:%d" % (what, dtype, self.device))
        return ctypes.c_void_p(t.data_ptr()), t.numel()

    def gather_dev(self, out, src, perm, stream=None):
        """sr_gather_batch_dev: out[t] = src[perm[t]] on whole ring elements (perm: int32 positions), out of place.  A position outside
        src is skipped and counted (spmv_bad_index_count).  Allocates nothing; capturable."""
        import torch

        w = self.words_per_elem
        po, no = self._dev_or_null(out)
        pi, ni = self._dev_or_null(src)
        pp, n = self._dev_idx(perm, torch.int32, "perm")
        if no != n * w or ni % w:
            raise RingError("gather: DifferentLengths")
        self._check(self._lib.sr_gather_batch_dev(self._ctx, po, pi, pp, n, ni // w, self._stream(stream)))
        return out

    def transpose_dev(self, out, a, nrows, ncols, stream=None):
        """sr_transpose_dev: out[j][i] = a[i][j] for a dense row-major nrows x ncols matrix, out of place.  Allocates nothing."""
        w = self.words_per_elem
        po, no = self._dev_or_null(out)
        pa, na = self._dev_or_null(a)
        if nrows < 0 or ncols < 0 or na != nrows * ncols * w or no != na:
            raise RingError("transpose: DifferentLengths")
        self._check(self._lib.sr_transpose_dev(self._ctx, po, pa, nrows, ncols, self._stream(stream)))
        return out

    def spgemm_ntt_dev(self, out_vals, live, a_vals, b_vals, pair_ptr, pair_a, pair_b, work=None, stream=None):
        """sr_spgemm_ntt_dev: out_vals[e] = sum of a_vals[pair_a[t]] * b_vals[pair_b[t]] over pair_ptr[e] <= t < pair_ptr[e + 1];
        live[e] (int32) = 1 iff some product of the entry is non-zero.  pair_ptr: int64 [n_out + 1], pair_a / pair_b: int32 (what
        spgemm_pattern wrote).  Entries that stay dead are counted (spgemm_dead_count).  Allocates nothing; capturable."""
        import torch

        w = self.words_per_elem
        po, no = self._dev_or_null(out_vals)
        pa, na = self._dev_or_null(a_vals)
        pb, nb = self._dev_or_null(b_vals)
        pw, nw = self._dev_or_null(work)
        pl, nl = self._dev_idx(live, torch.int32, "live")
        ppp, npp = self._dev_idx(pair_ptr, torch.int64, "pair_ptr")
        ppa, npa = self._dev_idx(pair_a, torch.int32, "pair_a")
        ppb, npb = self._dev_idx(pair_b, torch.int32, "pair_b")
        if npp < 1 or no != (npp - 1) * w or nl != npp - 1 or npa != npb or na % w or nb % w:
            raise RingError("spgemm: DifferentLengths")
        self._check(self._lib.sr_spgemm_ntt_dev(self._ctx, po, pl, pa, na // w, pb, nb // w, ppp, ppa, ppb, npp - 1, npa, pw, nw // w,
                                                self._stream(stream)))
        return out_vals

    def spgemm_dead_count(self, stream=None):
        """sr_spgemm_dead_count: the structural entries none of whose products was non-zero since the last read; clears the count."""
        n = ctypes.c_ulonglong(0)
        self._check(self._lib.sr_spgemm_dead_count(self._ctx, ctypes.byref(n), self._stream(stream)))
        return int(n.value)

    # ---- batch inversion (inverse.py holds the calls; the device form is inverse.inverse_dev(ring, ...), as lincomb_dev is) ----
    def inverse_plan(self, n, has_num=False):
        """sr_inverse_plan for this ring: (work_elems, launches, chunk_elems)."""
        from .inverse import inverse_plan

        return inverse_plan(self, n, has_num)

    def inverse(self, den, num=None):
        """Host buffers: sr_inverse_batch (see inverse_dev); returns the quotients as a new array."""
        from .inverse import inverse

        return inverse(self, den, num)

    def inverse_zero_count(self, stream=None):
        """sr_inverse_zero_count: the zero slots the inverse calls met since the last read; clears the count."""
        from .inverse import inverse_zero_count

        return inverse_zero_count(self, stream)

    def rot_dev(self, out, a, stream=None):
        po, n = self._dev(out)
        pa, m = self._dev(a)
        if n != m:
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_rot_batch_dev(self._ctx, po, pa, self._batch_of(n), self._stream(stream)))
        return out

    def gadget_decompose_dev(self, out, a, basis, padding_size, stream=None):
        po, n = self._dev(out)
        pa, m = self._dev(a)
        if n != m * padding_size:
            raise RingError("decompose: out must hold len * padding_size elements")
        lo, hi = _basis_words(basis, True)
        self._check(self._lib.sr_decompose_balanced_batch_wide_dev(self._ctx, po, pa, lo, hi, padding_size,
                                                                  self._batch_of(m), self._stream(stream)))
        return out

    def decompose_overflow_count(self, stream=None):
        n = ctypes.c_ulonglong(0)
        self._check(self._lib.sr_decompose_overflow_count(self._ctx, ctypes.byref(n), self._stream(stream)))
        return int(n.value)

    def gadget_recompose_dev(self, out, digits, basis, padding_size, stream=None):
        po, n = self._dev(out)
        pd, m = self._dev(digits)
        if m != n * padding_size:
            raise RingError("recompose: digits must hold len(out) * padding_size elements")
        lo, hi = _basis_words(basis, False)
        self._check(self._lib.sr_recompose_batch_wide_dev(self._ctx, po, pd, lo, hi, padding_size,
                                                         self._batch_of(n), self._stream(stream)))
        return out

    def serialize_dev(self, wire, a, offsets=None, stream=None):
        """wire: uint8 CUDA tensor; a: ring elements; offsets: optional int64 CUDA tensor, one byte offset (multiple of 8) per
        element, for callers that interleave framing words; None = densely packed."""
        import torch

        pa, n = self._dev(a)
        batch = self._batch_of(n)
        if wire.dtype != torch.uint8 or not wire.is_cuda or not wire.is_contiguous():
            raise RingError("serialize: wire must be a contiguous uint8 CUDA tensor")
        if offsets is None:
            if wire.numel() != batch * self.degree * self.wire_coeff_bytes:
                raise RingError("serialize: wire must hold len * D * wire_coeff_bytes bytes")
            po = 0
        else:
            if offsets.dtype != torch.int64 or offsets.numel() != batch or not offsets.is_cuda:
                raise RingError("serialize: offsets must be an int64 CUDA tensor with one entry per element")
            po = offsets.data_ptr()
        self._check(self._lib.sr_serialize_batch_dev(self._ctx, wire.data_ptr(), pa, po, batch, self._stream(stream)))
        return wire

    def deserialize_dev(self, out, wire, offsets=None, stream=None):
        """Inverse of serialize_dev; coefficients >= p are stored as 0 and counted (wire_invalid_count)."""
        import torch

        po_, n = self._dev(out)
        batch = self._batch_of(n)
        if wire.dtype != torch.uint8 or not wire.is_cuda or not wire.is_contiguous():
            raise RingError("deserialize: wire must be a contiguous uint8 CUDA tensor")
        if offsets is None:
            if wire.numel() != batch * self.degree * self.wire_coeff_bytes:
                raise RingError("deserialize: wire must hold len * D * wire_coeff_bytes bytes")
            po = 0
        else:
            if offsets.dtype != torch.int64 or offsets.numel() != batch or not offsets.is_cuda:
                raise RingError("deserialize: offsets must be an int64 CUDA tensor with one entry per element")
            po = offsets.data_ptr()
        self._check(self._lib.sr_deserialize_batch_dev(self._ctx, po_, wire.data_ptr(), po, batch, self._stream(stream)))
        return out

    def wire_invalid_count(self, stream=None):
        n = ctypes.c_ulonglong(0)
        self._check(self._lib.sr_wire_invalid_count(self._ctx, ctypes.byref(n), self._stream(stream)))
        return int(n.value)

    def mul_ntt_rhs(self, a, b_ntt):
        """Host buffers: icrt(crt(a) (.) b_ntt) with b_ntt = crt(b) already in CRT/NTT form; returns a new array."""
        if a.size != b_ntt.size:
            raise RingError("operand lengths differ")
        out = np.empty_like(a)
        self._check(self._lib.sr_ring_mul_ntt_rhs_batch(self._ctx, _np_ptr(out), _np_ptr(a), _np_ptr(b_ntt), self._batch_of(a.size)))
        return out

    def mul_ntt_rhs_dev(self, out, a, b_ntt, stream=None):
        """out = icrt(crt(a) (.) b_ntt) for b_ntt = crt(b) already in CRT/NTT form (the constant-operand product); a and b_ntt
        are only read; out may be a."""
        po, n = self._dev(out)
        pa, m = self._dev(a)
        pb, q = self._dev(b_ntt)
        if not (n == m == q):
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_ring_mul_ntt_rhs_batch_dev(self._ctx, po, pa, pb, self._batch_of(n), self._stream(stream)))
        return out

    def mul_dev(self, out, a, b, stream=None):
        """out = a * b (RqPoly * &RqPoly, coeff_form.rs:250-258); a and b are only read; out may be a."""
        po, n = self._dev(out)
        pa, m = self._dev(a)
        pb, q = self._dev(b)
        if not (n == m == q):
            raise RingError("operand lengths differ")
        self._check(self._lib.sr_ring_mul_batch_dev(self._ctx, po, pa, pb, self._batch_of(n), self._stream(stream)))
        return out

    def reduce_dev(self, out, coeffs, in_len_per_elem, stream=None):
        po, n = self._dev(out)
        pi, m = self._dev(coeffs)
        batch = self._batch_of(n)
        if m != batch * in_len_per_elem * self.limbs:
            raise RingError("reduce: buffer length does not match batch * in_len")
        self._check(self._lib.sr_reduce_batch_dev(self._ctx, pi, in_len_per_elem, po, batch, self._stream(stream)))
        return out

    def fill_uniform_dev(self, t, seed, first_coeff=0, stream=None):
        p, n = self._dev(t)
        if n % self.limbs:
            raise RingError("buffer is not a whole number of coefficients")
        self._check(self._lib.sr_fill_uniform_dev(self._ctx, seed, first_coeff, n // self.limbs, p, self._stream(stream)))
        return t

    def count_noncanonical_dev(self, t, stream=None):
        p, n = self._dev(t)
        c = ctypes.c_uint64()
        self._check(self._lib.sr_count_noncanonical_dev(self._ctx, p, n // self.limbs, ctypes.byref(c), self._stream(stream)))
        return c.value

    # -- twiddle sharing across GPUs (one RCCL broadcast at start-up) -------------------------
    def twiddle_block(self):
        p = ctypes.c_void_p()
        n = ctypes.c_size_t()
        self._check(self._lib.sr_ctx_twiddle_block(self._ctx, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def twiddles_updated(self):
        self._check(self._lib.sr_ctx_twiddles_updated(self._ctx))

    # -- per-kernel timing --------------------------------------------------------------------
    def profile_enable(self, on=True):
        """on: False / True (every launch bracketed by HIP events) or an int N >= 2 (every N-th launch only: leaves a two-lane step as
        it runs, see sr_ctx_profile_enable)"""
        self._check(self._lib.sr_ctx_profile_enable(self._ctx, int(on)))

    def profile_read(self):
        """per tag: ms and launches of the BRACKETED launches, seen = every launch that went by since the last read"""
        ms = (ctypes.c_double * len(PROF_TAGS))()
        n = (ctypes.c_uint64 * len(PROF_TAGS))()
        seen = (ctypes.c_uint64 * len(PROF_TAGS))()
        self._check(self._lib.sr_ctx_profile_read_sampled(self._ctx, ms, n, seen))
        return {t: {"ms": ms[i], "launches": int(n[i]), "seen": int(seen[i])} for i, t in enumerate(PROF_TAGS)}
