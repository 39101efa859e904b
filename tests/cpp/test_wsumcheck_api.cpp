// VirtualPolynomial::round_evals_weighted / ::fold_round_evals_weighted and EqSumCheck of include/stark_rings.hpp (sr_vpoly_wround_evals,
// sr_vpoly_wround_fold_evals: sum-check rounds with a per-pair weight) against the mirror's older calls: the explicit prover holds
// eq(z, .) as one more table of every product -- mul_by_mle, round_evals, fold_round_evals -- and must send, round by round, exactly the
// messages of EqSumCheck, for eq a b, R1CS  eq (a b - c)  and the fraction claim with a coefficient lambda (five tables in the explicit
// polynomial); all-one() weights against the unweighted calls; the plans; and the throws.  One shape per ring family, both orders.
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

// kind 0: a b; 1: a b - c; 2: p_lo q_hi + p_hi q_lo + lambda q_lo q_hi
static VirtualPolynomial claim(const CyclotomicConfig &cfg, size_t nv, const std::vector<Mle> &t, int kind, const RqNTTVec &minus_one,
                               const RqNTTVec &lambda) {
    VirtualPolynomial g(cfg, nv);
    if (kind == 0) {
        g.add_mle_list({&t[0], &t[1]});
    } else if (kind == 1) {
        g.add_mle_list({&t[0], &t[1]});
        g.add_mle_list({&t[2]}, &minus_one);
    } else {
        g.add_mle_list({&t[0], &t[3]});
        g.add_mle_list({&t[1], &t[2]});
        g.add_mle_list({&t[2], &t[3]}, &lambda);
    }
    return g;
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t full = (size_t)1 << nv, dim = cfg.dimension();
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    const RqNTTVec minus_one = -RqNTTVec(one), lambda(cfg, uniform(field, 0xA1, dim));
    std::vector<Mle> tabs;
    for (size_t j = 0; j < 4; j++) tabs.emplace_back(cfg, nv, uniform(field, 0x8E00 + j, (j == 1 ? full - 3 : full) * dim));
    const RqNTTVec z(cfg, uniform(field, 0x2E0, nv * dim));
    for (int kind = 0; kind < 3; kind++)
        for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
            const VirtualPolynomial g = claim(cfg, nv, tabs, kind, minus_one, lambda);
            const Mle eq(cfg, nv, eq_table(z).words());
            VirtualPolynomial e = claim(cfg, nv, tabs, kind, minus_one, lambda);
            e.mul_by_mle(&eq);
            EXPECT(e.degree() == g.degree() + 1 && e.tables().size() == g.tables().size() + 1);
            EqSumCheck prover(g, z, order);
            RqNTTVec msg = e.round_evals(order);
            for (size_t j = 0; j < nv; j++) {
                EXPECT(prover.message().words() == msg.words());
                EXPECT(prover.message().len() == g.degree() + 2 && prover.round() == j + 1);
                const RqNTTVec r(cfg, uniform(field, 0x7100 + j, dim));
                prover.next(r);
                if (j + 1 < nv) {
                    auto step = e.fold_round_evals(r, order);
                    msg = step.first;
                    e = step.second;
                } else {
                    e = e.fixed_variables(r, order);
                }
            }
            const auto fin = prover.final();
            EXPECT(fin.first.size() == g.tables().size());
            for (size_t j = 0; j < fin.first.size(); j++) EXPECT(fin.first[j].words() == e.tables()[j]->words());
            EXPECT(fin.second.words() == e.tables().back()->words());
        }
    // every weight one(): the unweighted calls, bit for bit
    const VirtualPolynomial g = claim(cfg, nv, tabs, 2, minus_one, lambda);
    Words ones;
    for (size_t b = 0; b < full / 2; b++) ones.insert(ones.end(), one.words().begin(), one.words().end());
    const RqNTTVec w1(cfg, ones), w2(cfg, Words(ones.begin(), ones.begin() + ones.size() / 2)), r(cfg, uniform(field, 5, dim));
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        EXPECT(g.round_evals_weighted(w1, order).words() == g.round_evals(order).words());
        auto got = g.fold_round_evals_weighted(r, w2, order);
        auto want = g.fold_round_evals(r, order);
        EXPECT(got.first.words() == want.first.words());
        for (size_t j = 0; j < 4; j++) EXPECT(got.second.tables()[j]->words() == want.second.tables()[j]->words());
        EXPECT(got.second.round_evals_weighted(w2, order).words() == got.first.words());
    }
    // the plans: host arithmetic
    for (int slots : {4, 8})
        for (int d = 1; d <= 4; d++) {
            const auto p = cfg.vpoly_wround_plan(log2d, nv, slots, 2, d, SR_MLE_LEADING), f = cfg.vpoly_wround_fold_plan(log2d, nv, slots, 2, d, SR_MLE_TRAILING);
            EXPECT((p.first == 0) == (p.second == 1) && (f.first == 0) == (f.second == 1));
        }
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    EXPECT(throws([&] { cfg.vpoly_wround_plan(log2d, nv, 4, 2, 3, SR_MLE_ROUND_SUM); }));
    EXPECT(throws([&] { cfg.vpoly_wround_fold_plan(log2d, 1, 4, 2, 3, SR_MLE_LEADING); }));
    EXPECT(throws([&] { g.round_evals_weighted(w2); }));                 // half the weights
    EXPECT(throws([&] { g.round_evals_weighted(w1, 2); }));
    EXPECT(throws([&] { g.fold_round_evals_weighted(r, w1); }));        // twice the weights
    EXPECT(throws([&] { g.fold_round_evals_weighted(w2, w2); }));       // r is not one element
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).round_evals_weighted(w1); }));
    EXPECT(throws([&] { EqSumCheck(g, r); }));                           // z has one element, not nv
    EXPECT(throws([&] { EqSumCheck(g, z, 2); }));
    EXPECT(throws([&] { EqSumCheck(g, z).final(); }));
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
