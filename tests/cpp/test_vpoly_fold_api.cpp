// VirtualPolynomial::fold_round_evals and ::fixed_variables of include/stark_rings.hpp (sr_vpoly_round_fold_evals: every distinct table
// folded at the challenge and the next round's message in one pass) against the composition of the mirror's older calls -- a fold per
// distinct table (fixed_variables / fix_last_variables), the polynomial rebuilt over the folded tables, round_evals -- for the
// structures R1CS  c0 e a b - e c  and REPEAT  c0 f0 f0 f1 f1 + c1 f1 + c2 f2 f3: one shape per ring family, both orders, a truncated
// table, bit for bit; a whole prover loop; one product without coefficients against DenseMultilinearExtension::fold_round_evals; and
// the throws.
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "../../include/stark_rings.hpp"
#include "../../oracle/sr_oracle.h"

using namespace stark_rings;
typedef std::vector<uint64_t> Words;
typedef DenseMultilinearExtension Mle;
typedef std::vector<std::vector<int>> Terms;

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

static VirtualPolynomial build(const CyclotomicConfig &cfg, size_t nv, const std::vector<Mle> &mles, const Terms &terms,
                               const std::vector<RqNTTVec> &coeffs) {
    VirtualPolynomial vp(cfg, nv);
    for (size_t k = 0; k < terms.size(); k++) {
        std::vector<const Mle *> ptrs;
        for (int j : terms[k]) ptrs.push_back(&mles[j]);
        vp.add_mle_list(ptrs, &coeffs[k]);
    }
    return vp;
}

// the stored part of `got` is the head of the whole folded table `want`, whose tail is zero
static bool folded_agrees(const Mle &got, const Mle &want) {
    const Words &g = got.words(), &x = want.words();
    if (got.num_vars() != want.num_vars() || g.size() > x.size()) return false;
    for (size_t i = 0; i < x.size(); i++)
        if (x[i] != (i < g.size() ? g[i] : 0)) return false;
    return true;
}

static void structure(const CyclotomicConfig &cfg, int field, size_t nv, const Terms &terms, size_t n_tables, uint64_t seed) {
    const size_t full = (size_t)1 << nv;
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    std::vector<Mle> mles;
    for (size_t j = 0; j < n_tables; j++) {
        const size_t n = j == 1 ? full - 3 : full;  // one truncated table
        mles.emplace_back(cfg, nv, uniform(field, seed + j, n * cfg.dimension()));
    }
    std::vector<RqNTTVec> coeffs;
    for (size_t k = 0; k < terms.size(); k++) coeffs.emplace_back(cfg, uniform(field, seed + 64 + k, cfg.dimension()));
    if (terms.size() == 2) coeffs[1] = -RqNTTVec(one);  // R1CS: c1 = -one()
    const VirtualPolynomial vp = build(cfg, nv, mles, terms, coeffs);
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        // a whole prover: round 0 from round_evals, rounds 1 .. nv - 1 from fold_round_evals, against the unfused loop
        VirtualPolynomial g = vp;
        std::vector<Mle> cur = mles;
        RqNTTVec msg = vp.round_evals(order);
        for (size_t left = nv; left >= 2; left--) {
            const RqNTTVec r(cfg, uniform(field, seed + 128 + left, cfg.dimension()));
            std::vector<Mle> next;
            for (const Mle &m : cur) next.push_back(order == SR_MLE_LEADING ? m.fixed_variables(r) : m.fix_last_variables(r));
            const RqNTTVec want = build(cfg, left - 1, next, terms, coeffs).round_evals(order);
            auto step = g.fold_round_evals(r, order);
            EXPECT(step.first.words() == want.words());
            EXPECT(step.second.num_vars() == left - 1 && step.second.tables().size() == n_tables && step.second.degree() == vp.degree());
            for (size_t j = 0; j < n_tables; j++) EXPECT(folded_agrees(*step.second.tables()[j], next[j]));
            for (size_t k = 0; k < terms.size(); k++)
                for (size_t s = 0; s < terms[k].size(); s++) EXPECT(step.second.terms()[k].table[s] == terms[k][s]);
            const VirtualPolynomial f = g.fixed_variables(r, order);  // no message
            EXPECT(f.num_vars() == left - 1 && f.tables().size() == n_tables);
            for (size_t j = 0; j < n_tables; j++) EXPECT(f.tables()[j]->words() == next[j].words());
            EXPECT(f.round_evals(order).words() == want.words());
            g = step.second;  // the folded tables live on in the copy
            cur = next;
            msg = step.first;
        }
        EXPECT(g.num_vars() == 1 && msg.len() == vp.degree() + 1);
        const RqNTTVec r(cfg, uniform(field, seed + 127, cfg.dimension()));
        const VirtualPolynomial last = g.fixed_variables(r, order);
        EXPECT(last.num_vars() == 0);
        for (size_t j = 0; j < n_tables; j++) {
            const Mle want = order == SR_MLE_LEADING ? cur[j].fixed_variables(r) : cur[j].fix_last_variables(r);
            EXPECT(last.tables()[j]->words() == want.words());
        }
    }
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t full = (size_t)1 << nv;
    structure(cfg, field, nv, {{0, 1, 2}, {0, 3}}, 4, 0x7E00);            // R1CS
    structure(cfg, field, nv, {{0, 0, 1, 1}, {1}, {2, 3}}, 4, 0x7F00);    // REPEAT
    // one product without coefficients is the fused round of a product, message and tables
    Mle e(cfg, nv, uniform(field, 1, full * cfg.dimension())), a(cfg, nv, uniform(field, 2, (full - 1) * cfg.dimension()));
    Mle b(cfg, nv, uniform(field, 3, (full / 2 + 1) * cfg.dimension())), tiny(cfg, 1, uniform(field, 4, 2 * cfg.dimension()));
    const RqNTTVec r(cfg, uniform(field, 5, cfg.dimension()));
    VirtualPolynomial single(cfg, nv);
    single.add_mle_list({&a, &b, &e});
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        auto got = single.fold_round_evals(r, order);
        auto want = Mle::fold_round_evals({&a, &b, &e}, r, order);
        EXPECT(got.first.words() == want.first.words());
        for (size_t j = 0; j < 3; j++) EXPECT(got.second.tables()[j]->words() == want.second[j].words());
    }
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    VirtualPolynomial one_var(cfg, 1);
    one_var.add_mle_list({&tiny});
    EXPECT(throws([&] { one_var.fold_round_evals(r); }));                         // the last round folds with fixed_variables
    EXPECT(one_var.fixed_variables(r).num_vars() == 0);
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).fold_round_evals(r); }));      // no product
    EXPECT(throws([&] { single.fold_round_evals(r, 2); }));
    EXPECT(throws([&] { single.fixed_variables(r, 2); }));
    EXPECT(throws([&] { single.fold_round_evals(RqNTTVec(cfg, uniform(field, 6, 2 * cfg.dimension()))); }));  // two elements
    EXPECT(throws([&] { one_var.fixed_variables(RqNTTVec(cfg, uniform(field, 6, 2 * cfg.dimension()))); }));  // too many points
    std::printf("%s ok\n", name);
}

int main() {
    family("goldilocks", SR_RING_GOLDILOCKS_POW2, SRO_GOLDILOCKS, 6, 6);
    family("babybear", SR_RING_BABYBEAR_POW2, SRO_BABYBEAR, 5, 5);
    family("stark", SR_RING_STARK_POW2, SRO_STARK, 4, 5);
    family("goldilocks24", SR_RING_GOLDILOCKS_24, SRO_GOLDILOCKS, 0, 6);
    family("babybear72", SR_RING_BABYBEAR_72, SRO_BABYBEAR, 0, 5);
    family("frog16", SR_RING_FROG_16, SRO_FROG, 0, 6);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
