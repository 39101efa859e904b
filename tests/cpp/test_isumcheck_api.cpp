// IndexMultilinearExtension, VirtualPolynomial::add_product / mul_by_mle over it and EqSumCheck over column factors of include/stark_rings.hpp
// (sr_vpoly_iwround_evals, sr_vpoly_iwround_fold_evals: weighted sum-check rounds whose factors may be integer columns) against the
// composition the header states: every column expanded with to_dense() (sr_lincomb_index) and the same claim run through the weighted
// calls over ring tables.  PLONK  q_L a + q_R b + q_M a b - q_O c + q_C  (3 tables, 5 selector columns: 0/1, the values around p,
// truncated, the two progressions) and ALLCOL (columns only, one of them twice in a term); the messages of EqSumCheck round by round, the
// folded slots, the final values, the expanding slow paths, the plan wrappers and the throws.  One shape per ring family, both orders.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../include/stark_rings.hpp"
#include "../../oracle/sr_oracle.h"

using namespace stark_rings;
typedef std::vector<uint64_t> Words;
typedef DenseMultilinearExtension Mle;
typedef IndexMultilinearExtension Imle;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static Words uniform(int field, uint64_t seed, size_t n_coeffs) {
    Words v(n_coeffs * sro_limbs(field));
    sro_fill_uniform(field, seed, 0, n_coeffs, v.data());
    return v;
}
static uint64_t next(uint64_t &s) {  // splitmix64
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the gate claim over tables a, b, c and selectors q (either kind of MLE): q_L a + q_R b + q_M a b - q_O c + q_C
static VirtualPolynomial plonk(const CyclotomicConfig &cfg, size_t nv, const std::vector<Mle> &t, const std::vector<Imle> &q, const RqNTTVec &minus_one) {
    VirtualPolynomial g(cfg, nv);
    g.add_product({&t[0]}, {&q[0]});
    g.add_product({&t[1]}, {&q[1]});
    g.add_product({&t[0], &t[1]}, {&q[2]});
    g.add_product({&t[2]}, {&q[3]}, &minus_one);
    g.add_product({}, {&q[4]});
    return g;
}
static VirtualPolynomial plonk_dense(const CyclotomicConfig &cfg, size_t nv, const std::vector<Mle> &t, const std::vector<Mle> &q, const RqNTTVec &minus_one) {
    VirtualPolynomial g(cfg, nv);
    g.add_mle_list({&t[0], &q[0]});
    g.add_mle_list({&t[1], &q[1]});
    g.add_mle_list({&t[0], &t[1], &q[2]});
    g.add_mle_list({&t[2], &q[3]}, &minus_one);
    g.add_mle_list({&q[4]});
    return g;
}

// g over columns and e, the same claim over expanded tables with the same slot order: every path of the two agrees word for word
static void same_prover(const CyclotomicConfig &cfg, int field, size_t nv, const VirtualPolynomial &g, const VirtualPolynomial &e) {
    const size_t dim = cfg.dimension(), full = (size_t)1 << nv;
    EXPECT(g.has_columns() && !e.has_columns() && g.tables().size() == e.tables().size() && g.degree() == e.degree());
    const RqNTTVec z(cfg, uniform(field, 0x2E0, nv * dim)), r0(cfg, uniform(field, 0x51, dim));
    const RqNTTVec w1(cfg, uniform(field, 0x3E1, full / 2 * dim));
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        // the two calls themselves
        EXPECT(g.round_evals_weighted(w1, order).words() == e.round_evals_weighted(w1, order).words());
        if (nv >= 2) {
            const RqNTTVec w2(cfg, uniform(field, 0x3E2, full / 4 * dim));
            auto got = g.fold_round_evals_weighted(r0, w2, order);
            auto want = e.fold_round_evals_weighted(r0, w2, order);
            EXPECT(got.first.words() == want.first.words() && !got.second.has_columns() && got.second.num_vars() == nv - 1);
            EXPECT(got.second.tables().size() == want.second.tables().size());
            for (size_t j = 0; j < want.second.tables().size(); j++) EXPECT(got.second.tables()[j]->words() == want.second.tables()[j]->words());
            // the slow paths expand
            auto slow = g.fold_round_evals(r0, order);
            auto slow_want = e.fold_round_evals(r0, order);
            EXPECT(slow.first.words() == slow_want.first.words());
        }
        EXPECT(g.round_evals(order).words() == e.round_evals(order).words());
        EXPECT(g.fixed_variables(r0, order).tables()[0]->words() == e.fixed_variables(r0, order).tables()[0]->words());
        // a whole sum-check, round by round
        EqSumCheck prover(g, z, order), explicit_prover(e, z, order);
        for (size_t j = 0; j < nv; j++) {
            EXPECT(prover.message().words() == explicit_prover.message().words());
            EXPECT(prover.message().len() == g.degree() + 2);
            const RqNTTVec r(cfg, uniform(field, 0x7100 + j, dim));
            prover.next(r);
            explicit_prover.next(r);
        }
        const auto fin = prover.final(), want = explicit_prover.final();
        EXPECT(fin.first.size() == g.tables().size() && fin.second.words() == want.second.words());
        for (size_t j = 0; j < fin.first.size(); j++) EXPECT(fin.first[j].words() == want.first[j].words());
    }
    EXPECT(g.sum().words() == e.sum().words());
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv, uint64_t p /* 0: above 2^64 */) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t full = (size_t)1 << nv, dim = cfg.dimension();
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    const RqNTTVec minus_one = -RqNTTVec(one);
    std::vector<Mle> tabs;
    for (size_t j = 0; j < 3; j++) tabs.emplace_back(cfg, nv, uniform(field, 0x8E00 + j, (j == 1 ? full - 3 : full) * dim));
    uint64_t seed = 0x15C0 + nv;
    Words bits(full), edge(full - 1), some(full / 2 + 1);
    const uint64_t around[4] = {p - 1, p, p + 1, UINT64_MAX};  // p == 0: 2^64 - 1, 0, 1, 2^64 - 1
    for (auto &x : bits) x = next(seed) & 1;
    for (size_t i = 0; i < edge.size(); i++) edge[i] = around[i % 4];
    for (auto &x : some) x = next(seed);
    std::vector<Imle> q;
    q.emplace_back(cfg, nv, IndexColumn::stored(bits));
    q.emplace_back(cfg, nv, IndexColumn::stored(edge));
    q.emplace_back(cfg, nv, IndexColumn::progression(0));
    q.emplace_back(cfg, nv, IndexColumn::stored(some));
    q.emplace_back(cfg, nv, IndexColumn::progression(UINT64_MAX - (full - 1)));  // the last legal start
    std::vector<Mle> qd;
    for (const Imle &c : q) qd.push_back(c.to_dense());
    EXPECT(q[1].len() == full - 1 && q[2].len() == full && qd[3].len() == full / 2 + 1 && qd[4].num_vars() == nv);
    // to_dense is from_u64: R::from(0) = zero(), R::from(1) = one()
    EXPECT(Words(qd[2].words().begin(), qd[2].words().begin() + cfg.words_per_elem()) == Words(cfg.words_per_elem(), 0));
    EXPECT(Words(qd[2].words().begin() + cfg.words_per_elem(), qd[2].words().begin() + 2 * cfg.words_per_elem()) == one.words());
    // PLONK: the 8-slot class
    const VirtualPolynomial g = plonk(cfg, nv, tabs, q, minus_one), e = plonk_dense(cfg, nv, tabs, qd, minus_one);
    EXPECT(g.tables().size() == 8 && g.degree() == 3);
    same_prover(cfg, field, nv, g, e);
    // ALLCOL: no table at all, one column twice in a term, mul_by_mle with a column
    VirtualPolynomial a(cfg, nv), ad(cfg, nv);
    a.add_product({}, {&q[1], &q[1]});
    a.add_product({}, {&q[0]}, &minus_one);
    a.mul_by_mle(&q[4]);
    ad.add_mle_list({&qd[1], &qd[1]});
    ad.add_mle_list({&qd[0]}, &minus_one);
    ad.mul_by_mle(&qd[4]);
    EXPECT(a.tables().size() == 3 && a.degree() == 3 && a.columns().size() == 3 && a.tables()[0] == nullptr);
    same_prover(cfg, field, nv, a, ad);
    // one variable: EqSumCheck's only fold goes through fixed_variables
    {
        std::vector<Imle> c1;
        c1.emplace_back(cfg, 1, IndexColumn::stored({7, UINT64_MAX}));
        c1.emplace_back(cfg, 1, IndexColumn::progression(UINT64_MAX - 1));
        const Mle d0 = c1[0].to_dense(), d1 = c1[1].to_dense();
        VirtualPolynomial s(cfg, 1), sd(cfg, 1);
        s.add_product({}, {&c1[0], &c1[1]});
        sd.add_mle_list({&d0, &d1});
        same_prover(cfg, field, 1, s, sd);
    }
    // the plan wrappers: the weighted plan at K + J slots
    for (int d = 1; d <= 4; d++) {
        EXPECT(cfg.vpoly_iwround_plan(log2d, nv, 3, 5, 5, d, SR_MLE_LEADING, false) == cfg.vpoly_wround_plan(log2d, nv, 8, 5, d, SR_MLE_LEADING));
        EXPECT(cfg.vpoly_iwround_plan(log2d, nv, 0, 2, 1, d, SR_MLE_TRAILING, true) == cfg.vpoly_wround_fold_plan(log2d, nv, 2, 1, d, SR_MLE_TRAILING));
    }
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    EXPECT(throws([&] { cfg.vpoly_iwround_plan(log2d, nv, 4, 5, 2, 3, SR_MLE_LEADING, false); }));   // nine slots
    EXPECT(throws([&] { cfg.vpoly_iwround_plan(log2d, nv, 1, 9, 2, 3, SR_MLE_LEADING, false); }));
    EXPECT(throws([&] { cfg.vpoly_iwround_plan(log2d, 1, 1, 1, 2, 3, SR_MLE_LEADING, true); }));
    EXPECT(throws([&] { Imle(cfg, nv, IndexColumn::progression(UINT64_MAX - (full - 2))); }));       // wraps past 2^64 - 1
    EXPECT(throws([&] { Imle(cfg, nv, IndexColumn::stored(Words(full + 1, 1))); }));
    EXPECT(throws([&] { Imle(cfg, 48, IndexColumn::progression(0)); }));
    const Imle other(cfg, nv + 1, IndexColumn::progression(0));
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).add_product({}, {&other}); }));                 // another num_vars
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).add_product({&tabs[0], &tabs[1], &tabs[2]}, {&q[0], &q[1]}); }));  // five factors
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).add_product({}, {}); }));
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).mul_by_mle(&q[0]); }));                           // an empty polynomial
    VirtualPolynomial nine = plonk(cfg, nv, tabs, q, minus_one);
    const Imle extra(cfg, nv, IndexColumn::progression(5));
    EXPECT(throws([&] { nine.add_product({}, {&extra}); }) && nine.tables().size() == 8 && nine.terms().size() == 5);  // a ninth slot, nothing changed
    EXPECT(throws([&] { g.round_evals_weighted(RqNTTVec(cfg, uniform(field, 1, dim))); }) || nv == 1);   // one weight, not one per pair
    std::printf("%s ok\n", name);
}

int main() {
    family("goldilocks", SR_RING_GOLDILOCKS_POW2, SRO_GOLDILOCKS, 6, 5, 0xFFFFFFFF00000001ull);
    family("babybear", SR_RING_BABYBEAR_POW2, SRO_BABYBEAR, 5, 5, 2013265921ull);
    family("stark", SR_RING_STARK_POW2, SRO_STARK, 4, 4, 0);
    family("goldilocks24", SR_RING_GOLDILOCKS_24, SRO_GOLDILOCKS, 0, 5, 0xFFFFFFFF00000001ull);
    family("babybear72", SR_RING_BABYBEAR_72, SRO_BABYBEAR, 0, 4, 2013265921ull);
    family("frog16", SR_RING_FROG_16, SRO_FROG, 0, 5, 15912092521325583641ull);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
