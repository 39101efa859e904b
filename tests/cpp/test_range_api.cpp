// RangePolynomial, RangeSumCheck and the three range_wround_* calls of include/stark_rings.hpp (sr_range_wround_plan, sr_range_wround_evals:
// the norm check sum_b eq(beta, b) sum_i mu_i prod_{|j| < B} (f_i(b) - j) from one read of each table) against the mirror's older calls:
// at bound 2 the VirtualPolynomial of (f, f - 1, f + 1) with one product of three factors per table must give, round by round, exactly the
// messages of RangeSumCheck; an honest witness gives h(0) = h(1) = 0 at bounds 2, 3 and 8; the plans; and the throws.  One shape per ring
// family, both orders.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../include/stark_rings.hpp"
#include "../../oracle/sr_oracle.h"

using namespace stark_rings;
typedef std::vector<uint64_t> Words;
typedef DenseMultilinearExtension Mle;

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
static RqNTTVec repeat(const CyclotomicConfig &cfg, const RqNTTVec &e, size_t n) {
    Words v;
    for (size_t i = 0; i < n; i++) v.insert(v.end(), e.words().begin(), e.words().end());
    return RqNTTVec(cfg, v);
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t full = (size_t)1 << nv, dim = cfg.dimension();
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    const RqNTTVec ones = repeat(cfg, one, full);
    // two tables, their shifts, coefficients
    std::vector<Mle> f, shifted;
    for (size_t i = 0; i < 2; i++) {
        const RqNTTVec t(cfg, uniform(field, 0x9E00 + i, full * dim));
        RqNTTVec lo = t, hi = t;
        lo -= ones;
        hi += ones;
        f.emplace_back(cfg, nv, t.words());
        shifted.emplace_back(cfg, nv, t.words());
        shifted.emplace_back(cfg, nv, lo.words());
        shifted.emplace_back(cfg, nv, hi.words());
    }
    const RqNTTVec mu(cfg, uniform(field, 0xA7, 2 * dim)), z(cfg, uniform(field, 0x2E1, nv * dim));
    const RqNTTVec mu0(cfg, Words(mu.words().begin(), mu.words().begin() + mu.words().size() / 2)),
        mu1(cfg, Words(mu.words().begin() + mu.words().size() / 2, mu.words().end()));
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        VirtualPolynomial e(cfg, nv);
        e.add_mle_list({&shifted[0], &shifted[1], &shifted[2]}, &mu0);
        e.add_mle_list({&shifted[3], &shifted[4], &shifted[5]}, &mu1);
        const RangePolynomial g(cfg, {&f[0], &f[1]}, 2, &mu);
        EXPECT(g.degree() == 3 && e.degree() == 3 && g.num_vars() == nv && g.tables().size() == 2);
        EqSumCheck want(e, z, order);
        RangeSumCheck got(g, z, order);
        for (size_t j = 0; j < nv; j++) {
            EXPECT(got.message().words() == want.message().words());
            EXPECT(got.message().len() == 5 && got.round() == j + 1);
            const RqNTTVec r(cfg, uniform(field, 0x7300 + j, dim));
            got.next(r);
            want.next(r);
        }
        const auto a = got.final(), b = want.final();
        EXPECT(a.second.words() == b.second.words() && a.first.size() == 2 && b.first.size() == 6);
        for (size_t i = 0; i < 2; i++) EXPECT(a.first[i].words() == b.first[3 * i].words());
    }
    // an honest witness: every slot of every element one of -1, 0, 1; every bound from 2 on gives h(0) = h(1) = 0
    Words honest;
    const RqNTTVec zero(cfg, Words(one.words().size(), 0)), minus_one = -RqNTTVec(one);
    for (size_t b = 0; b < full; b++) {
        const RqNTTVec &c = b % 3 == 0 ? one : b % 3 == 1 ? zero : minus_one;
        honest.insert(honest.end(), c.words().begin(), c.words().end());
    }
    const Mle h(cfg, nv, honest);
    const RqNTTVec w(cfg, uniform(field, 0xEE, (full / 2) * dim));
    for (int bound : {2, 3, 8})
        for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
            const RqNTTVec msg = RangePolynomial(cfg, {&h}, bound).round_evals_weighted(w, order);
            EXPECT(msg.len() == (size_t)(2 * bound));
            bool zero01 = true;
            for (size_t i = 0; i < 2 * one.words().size(); i++) zero01 = zero01 && msg.words()[i] == 0;
            EXPECT(zero01);
        }
    // the plans: host arithmetic
    for (int bound = 2; bound <= 8; bound++) {
        const auto p = cfg.range_wround_plan(log2d, nv, 3, bound, SR_MLE_LEADING);
        EXPECT((p.first == 0) == (p.second == 1) && p.first % (2 * bound) == 0);
    }
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    const RangePolynomial g(cfg, {&f[0], &f[1]}, 3);
    const RqNTTVec wh(cfg, Words(w.words().begin(), w.words().begin() + w.words().size() / 2)), r(cfg, uniform(field, 5, dim));
    EXPECT(throws([&] { cfg.range_wround_plan(log2d, nv, 3, 9, SR_MLE_LEADING); }));
    EXPECT(throws([&] { cfg.range_wround_plan(log2d, nv, 9, 2, SR_MLE_LEADING); }));
    EXPECT(throws([&] { cfg.range_wround_plan(log2d, 0, 3, 2, SR_MLE_LEADING); }));
    EXPECT(throws([&] { cfg.range_wround_plan(log2d, nv, 3, 2, SR_MLE_ROUND_SUM); }));
    EXPECT(throws([&] { RangePolynomial(cfg, {&f[0]}, 1); }));
    EXPECT(throws([&] { RangePolynomial(cfg, {}, 2); }));
    EXPECT(throws([&] { RangePolynomial(cfg, {&f[0], &f[1]}, 2, &mu0); }));  // one coefficient for two tables
    EXPECT(throws([&] { g.round_evals_weighted(wh); }));                      // half the weights
    EXPECT(throws([&] { g.round_evals_weighted(w, 2); }));
    EXPECT(throws([&] { g.fold_round_evals_weighted(w, wh); }));              // r is not one element
    EXPECT(throws([&] { RangeSumCheck(g, r); }));                             // z has one element, not nv
    EXPECT(throws([&] { RangeSumCheck(g, z).final(); }));
    const auto step = g.fold_round_evals_weighted(r, wh, SR_MLE_TRAILING);
    EXPECT(step.second.num_vars() == nv - 1 && step.first.words() == step.second.round_evals_weighted(wh, SR_MLE_TRAILING).words());
    EXPECT(step.second.tables()[1]->words() == f[1].fix_last_variables(r).words());
    std::printf("%s ok\n", name);
}

int main() {
    family("goldilocks", SR_RING_GOLDILOCKS_POW2, SRO_GOLDILOCKS, 6, 5);
    family("babybear", SR_RING_BABYBEAR_POW2, SRO_BABYBEAR, 5, 5);
    family("stark", SR_RING_STARK_POW2, SRO_STARK, 4, 4);
    family("goldilocks24", SR_RING_GOLDILOCKS_24, SRO_GOLDILOCKS, 0, 5);
    family("babybear72", SR_RING_BABYBEAR_72, SRO_BABYBEAR, 0, 4);
    family("frog16", SR_RING_FROG_16, SRO_FROG, 0, 5);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
