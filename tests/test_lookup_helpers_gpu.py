"""logUp in its helper-column form (LookupHelperColumns) on goldilocks D = 2^6 and goldilocks24: 2^5 witness rows looked up in 2^3 table
rows from u64 indices.  The helper columns are the inverse columns (checked slot by slot through the model's product), their sums are
the values P/Q of the two fraction trees (FractionTree.root_value), and both zero claims h q - num run through EqSumCheck and are read
by the plain verifier of tests/protocol_verifier.py.  Also DenseMultilinearExtension.inverse / .divide, and root_value's refusal."""
import numpy as np
import pytest

from protocol_verifier import same
from stark_rings_amd import inverse_dev
from test_mle_gpu import dev, host, model_for
from test_protocols_gpu import Draw, claimed_sum, drive, env_for, g_of_terms, slots_of

pytestmark = pytest.mark.gpu
CHECKS = [("goldilocks", 6), ("goldilocks24", 0)]
IDS = [c[0] for c in CHECKS]
NV_W, NV_T = 5, 3
TRAILING = 1


@pytest.fixture(scope="module")
def torch_cuda():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


class Setup:
    def __init__(self, torch, name, k):
        from stark_rings_amd import fingerprint

        self.torch = torch
        self.env = env_for(torch, name, k)
        self.md = md = model_for(name, k)
        self.ring, self.w = md.ring, md.w
        n_t, n_w = 1 << NV_T, 1 << NV_W
        rng = np.random.RandomState(0x10C)
        self.col = md.uniform(0xF000, n_t).reshape(n_t, md.w)
        self.picks = rng.randint(0, n_t, n_w).astype(np.uint64)
        self.picks[:n_t] = np.arange(n_t, dtype=np.uint64)
        zero, one = md.zero(), md.elems(md.one())[0]
        self.minus = dev(torch, md.words([md.sub(zero, one)]))
        self.fingerprint = fingerprint

    def q(self, rows, beta):
        """beta - row, for every row"""
        return self.fingerprint(self.ring, [dev(self.torch, np.ascontiguousarray(rows).reshape(-1))], self.minus, beta)

    def columns(self, beta, witness_rows=None):
        from stark_rings_amd import LookupHelperColumns

        rows = self.col[self.picks.astype(np.int64)] if witness_rows is None else witness_rows
        self.q_w, self.q_t = self.q(rows, beta), self.q(self.col, beta)
        return LookupHelperColumns.from_indices(self.ring, self.q_w, self.q_t, dev(self.torch, self.picks), NV_W, NV_T)


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_helper_columns_hold_and_their_sums_are_the_fraction_trees_values(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import LookupCheck

    s = Setup(torch, name, k)
    env, V, ring = s.env, s.env.V, s.ring
    ring.inverse_zero_count()
    beta = dev(torch, s.md.uniform(0xF020, 1))
    lh = s.columns(beta)
    assert lh.zero_slots == 0 and lh.holds()
    # the columns are the inverse columns: h q == num in the model's arithmetic, row by row
    h_w, h_t, q_w, q_t, m = (env.get(t) for t in (lh.h_w, lh.h_t, s.q_w, s.q_t, lh.multiplicities))
    assert all(same(V.mul(h, q), V.one) for h, q in zip(h_w, q_w))
    assert all(same(V.mul(h, q), mj) for h, q, mj in zip(h_t, q_t, m))
    counts = np.bincount(s.picks.astype(np.int64), minlength=1 << NV_T)
    assert all(same(mj, V.scalar(int(c))) for mj, c in zip(m, counts))
    # sum h_w = P_w / Q_w and sum h_t = P_t / Q_t of the fraction trees over the same leaves
    lc = LookupCheck.from_indices(ring, s.q_w, s.q_t, dev(torch, s.picks), NV_W, NV_T)
    assert lc.holds()
    sw, st = lh.sums()
    assert np.array_equal(host(sw), host(lc.witness.root_value())) and np.array_equal(host(st), host(lc.table.root_value()))
    assert same(env.get(sw)[0], V.sum(h_w)) and same(env.get(st)[0], V.sum(h_t))
    assert ring.inverse_zero_count() == 0


def verify_zero_claim(s, lh, side, *key):
    """EqSumCheck over zero_claim(side), read by the plain verifier; the claimed sum is zero"""
    from stark_rings_amd import EqSumCheck

    env, V = s.env, s.env.V
    g = lh.zero_claim(side)
    nv = NV_T if side else NV_W
    held = [lh.h_t, lh.table_q, lh.multiplicities] if side else [lh.h_w, lh.witness_q, lh.ones]

    class T:   # what slots_of reads
        def __init__(self, t):
            self.evaluations = t

    tables = [env.get(t) for t in held]
    terms, coeffs = [[0, 1], [2]], [None, V.sub(V.zero, V.one)]
    g_of = g_of_terms(V, terms, coeffs)
    d = Draw(env, "helper", side, *key)
    z, _ = d.z(nv, False)
    claim0 = claimed_sum(V, z, nv, lambda b: g_of([t[b] for t in tables]))
    assert same(claim0, V.zero)
    challenges = d.challenges(nv)
    msgs, finals, eq_r = drive(env, EqSumCheck(g, env.put(z), TRAILING), challenges, slots_of(g, [T(t) for t in held]))
    V.verify_eq_sumcheck(V.zero, z, msgs, challenges, finals, eq_r, TRAILING, g_of, tables, points=4)


@pytest.mark.parametrize("side", (0, 1), ids=("witness", "table"))
@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_the_zero_claims_verify(torch_cuda, name, k, side):
    torch = torch_cuda
    s = Setup(torch, name, k)
    lh = s.columns(dev(torch, s.md.uniform(0xF021, 1)))
    verify_zero_claim(s, lh, side, name)


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_a_truncated_side_is_refused(torch_cuda, name, k):
    """n_w < 2^num_vars_w or n_t < 2^num_vars_t: refused by the constructor and by from_indices, whichever side it is, by the count
    given or by the length of the column"""
    torch = torch_cuda
    from stark_rings_amd import LookupHelperColumns, RingError

    s = Setup(torch, name, k)
    ring, w = s.ring, s.w
    beta = dev(torch, s.md.uniform(0xF024, 1))
    q_w, q_t = s.q(s.col[s.picks.astype(np.int64)], beta), s.q(s.col, beta)
    mult = dev(torch, s.md.uniform(0xF025, 1 << NV_T))
    idx = dev(torch, s.picks)
    LookupHelperColumns(ring, q_w, q_t, mult, NV_W, NV_T)                      # the full form is taken
    for kwargs in ({"n_w": (1 << NV_W) - 1}, {"n_t": (1 << NV_T) - 1}, {"n_w": 1, "n_t": 1}):
        with pytest.raises(RingError, match="truncated"):
            LookupHelperColumns(ring, q_w, q_t, mult, NV_W, NV_T, **kwargs)
        with pytest.raises(RingError, match="truncated"):
            LookupHelperColumns.from_indices(ring, q_w, q_t, idx, NV_W, NV_T, **kwargs)
    with pytest.raises(RingError, match="truncated"):                          # a witness column one row short, no count given
        LookupHelperColumns(ring, q_w[:-w], q_t, mult, NV_W, NV_T)
    with pytest.raises(RingError, match="truncated"):                          # a table column one row short
        LookupHelperColumns.from_indices(ring, q_w, q_t[:-w], idx, NV_W, NV_T)
    with pytest.raises(RingError, match="truncated"):                          # more variables than the columns fill
        LookupHelperColumns(ring, q_w, q_t, mult, NV_W + 1, NV_T)
    torch.cuda.synchronize()
    ring.spmv_bad_index_count()   # from_indices counted before it was refused: indices at or past a shortened table are skipped and counted


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_the_padded_full_form_of_a_truncated_lookup(torch_cuda, name, k):
    """29 witness rows of 2^5 and 6 table rows of 2^3, the padding written out as the class asks: q = one() on both sides, m = zero().
    The helper columns are 1 resp. 0 on the padded rows, both zero claims verify, sum h_t and sum h_w less the padded rows are the
    values of the truncated fraction trees, and the lookup holds after that correction; with the witness padded by copies of a table
    row that the multiplicities count, holds() is true as it stands."""
    torch = torch_cuda
    from stark_rings_amd import FractionTree, LookupHelperColumns

    s = Setup(torch, name, k)
    env, V, ring, w, md = s.env, s.env.V, s.ring, s.w, s.md
    ring.inverse_zero_count()
    n_w, n_t = 29, 6
    pad_w, pad_t = (1 << NV_W) - n_w, (1 << NV_T) - n_t
    picks = s.picks[:n_w] % n_t
    beta = dev(torch, md.uniform(0xF026, 1))
    one = dev(torch, md.one())
    q_w_real, q_t_real = s.q(s.col[picks.astype(np.int64)], beta), s.q(s.col[:n_t], beta)
    q_w, q_t = torch.cat([q_w_real, one.repeat(pad_w)]), torch.cat([q_t_real, one.repeat(pad_t)])
    lh = LookupHelperColumns.from_indices(ring, q_w, q_t, dev(torch, picks), NV_W, NV_T)
    assert lh.zero_slots == 0
    assert not host(lh.multiplicities)[n_t * w:].any()                                         # m = zero() on the padded table rows
    assert not host(lh.h_t)[n_t * w:].any()                                                    # h = 0 there
    assert np.array_equal(host(lh.h_w)[n_w * w:], np.tile(md.one(), pad_w))                    # h = 1 on the padded witness rows
    for side in (0, 1):
        verify_zero_claim(s, lh, side, name, "padded")
    sw, st = (env.get(t)[0] for t in lh.sums())
    sw_real = V.sub(sw, V.scalar(pad_w))
    assert same(sw_real, st) and not lh.holds()                                                # the padded rows are in sum h_w
    tw, tt = FractionTree(ring, None, q_w_real, NV_W, n_w), FractionTree(ring, lh.multiplicities, q_t_real, NV_T, n_t)
    assert same(env.get(tw.root_value())[0], sw_real) and same(env.get(tt.root_value())[0], st)
    # the other padding: copies of table row 0, counted
    picks2 = np.concatenate([picks, np.zeros(pad_w, dtype=np.uint64)])
    lh2 = LookupHelperColumns.from_indices(ring, s.q(s.col[picks2.astype(np.int64)], beta), q_t, dev(torch, picks2), NV_W, NV_T)
    assert lh2.zero_slots == 0 and lh2.holds()
    assert ring.inverse_zero_count() == 0


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_a_wrong_witness_row_and_a_challenge_on_a_table_value_fail(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import FractionTree, RingError

    s = Setup(torch, name, k)
    ring = s.ring
    ring.inverse_zero_count()
    beta = dev(torch, s.md.uniform(0xF022, 1))
    rows = s.col[s.picks.astype(np.int64)].copy()
    rows[20] = s.md.uniform(0xF023, 1)          # a witness row that is not in the table
    lh = s.columns(beta, rows)
    assert lh.zero_slots == 0 and not lh.holds()
    # beta equal to a table value: that row's denominator is zero in every slot, and so is every witness row taken from it
    hit = s.columns(dev(torch, s.col[3].copy()))
    n_slots = s.env.n_slots()
    assert hit.zero_slots == n_slots * (1 + int((s.picks == 3).sum())) and not hit.holds()
    assert not host(hit.h_t)[3 * s.w:4 * s.w].any()
    # the tree over the same leaves has a zero Q: no value, and the refusal neither counts nor clears
    z = dev(torch, np.zeros(2 * s.w, dtype=np.uint64))
    inverse_dev(ring, torch.empty_like(z), z)      # leaves 2 elements' slots in the count, unread
    tree = FractionTree(ring, None, s.q_t, NV_T)
    with pytest.raises(RingError, match="zero slot"):
        tree.root_value()
    good = FractionTree(ring, None, s.q(s.col, beta), NV_T)
    good.root_value()
    torch.cuda.synchronize()
    assert ring.inverse_zero_count() == 2 * n_slots


@pytest.mark.parametrize("name,k", CHECKS, ids=IDS)
def test_mle_inverse_and_divide(torch_cuda, name, k):
    torch = torch_cuda
    from stark_rings_amd import DenseMultilinearExtension as MLE, RingError

    s = Setup(torch, name, k)
    env, V, ring = s.env, s.env.V, s.ring
    ring.inverse_zero_count()
    a_words, b_words = s.md.uniform(0xF030, 13), s.md.uniform(0xF031, 13)    # 13 of 2^4 evaluations stored
    a, b = MLE(ring, 4, dev(torch, a_words)), MLE(ring, 4, dev(torch, b_words))
    inv, quo = b.inverse(), a.divide(b)
    assert inv.num_vars == quo.num_vars == 4 and len(inv) == len(quo) == 13
    am, bm = env.get(a.evaluations), env.get(b.evaluations)
    assert all(same(V.mul(x, y), V.one) for x, y in zip(env.get(inv.evaluations), bm))
    assert all(same(V.mul(x, y), n) for x, y, n in zip(env.get(quo.evaluations), bm, am))
    assert np.array_equal(host(a.evaluations), a_words) and np.array_equal(host(b.evaluations), b_words)
    assert ring.inverse_zero_count() == 0
    with pytest.raises(RingError, match="stored length"):
        a.divide(MLE(ring, 4, dev(torch, b_words[:12 * s.w])))
    empty = MLE(ring, 3, torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert len(empty.inverse()) == 0
