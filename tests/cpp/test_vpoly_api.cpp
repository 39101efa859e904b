// VirtualPolynomial of include/stark_rings.hpp (sr_vpoly_round_evals: a sum of products of dense MLEs with ring coefficients in one
// pass) against the composition of the mirror's older calls, for the structures R1CS  c0 e a b - e c  and REPEAT  c0 f0 f0 f1 f1 +
// c1 f1 + c2 f2 f3: every table folded at the point [t * one] (fixed_variables / fix_last_variables; one() is eq_table of the empty
// point), per term the folded tables multiplied slot-wise (sr_pointwise_mul_batch), summed (sr_sum_batch), scaled by the coefficient
// (mul_assign_elem) and added -- one shape per ring family, both orders, a truncated table, bit for bit; the slots of shared tables;
// and the throws at the limits.
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

typedef std::vector<std::vector<int>> Terms;

// sum_k c_k sum_b prod_s tables[terms[k][s]][b] from the older calls; every table holds all `n` elements
static Words sum_of_terms(const CyclotomicConfig &cfg, const std::vector<Words> &tables, const Terms &terms, const std::vector<RqNTTVec> &coeffs,
                          size_t n) {
    Words total(cfg.words_per_elem(), 0);
    for (size_t k = 0; k < terms.size(); k++) {
        Words acc = tables[terms[k][0]];
        for (size_t s = 1; s < terms[k].size(); s++)
            CyclotomicConfig::check(sr_pointwise_mul_batch(cfg.raw(), acc.data(), tables[terms[k][s]].data(), n), "pointwise");
        RqNTTVec part = RqNTTVec(cfg, acc).sum();
        part.mul_assign_elem(coeffs[k]);
        CyclotomicConfig::check(sr_add_batch(cfg.raw(), total.data(), part.words().data(), 1), "add");
    }
    return total;
}

static void structure(const CyclotomicConfig &cfg, int field, size_t nv, const Terms &terms, size_t n_tables, uint64_t seed) {
    const size_t w = cfg.words_per_elem(), full = (size_t)1 << nv;
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    std::vector<Mle> mles;
    for (size_t j = 0; j < n_tables; j++) {
        const size_t n = j == 1 ? full - 3 : full;  // one truncated table
        mles.emplace_back(cfg, nv, uniform(field, seed + j, n * cfg.dimension()));
    }
    std::vector<RqNTTVec> coeffs;
    for (size_t k = 0; k < terms.size(); k++) coeffs.emplace_back(cfg, uniform(field, seed + 64 + k, cfg.dimension()));
    if (terms.size() == 2) coeffs[1] = -RqNTTVec(one);  // R1CS: c1 = -one()
    VirtualPolynomial vp(cfg, nv);
    size_t degree = 0;
    for (size_t k = 0; k < terms.size(); k++) {
        std::vector<const Mle *> ptrs;
        for (int j : terms[k]) ptrs.push_back(&mles[j]);
        vp.add_mle_list(ptrs, &coeffs[k]);
        degree = terms[k].size() > degree ? terms[k].size() : degree;
    }
    EXPECT(vp.tables().size() == n_tables);  // a table shared between terms, or twice in one, is one slot
    EXPECT(vp.degree() == degree);
    std::vector<Words> whole;
    for (const Mle &m : mles) whole.push_back(m.to_evaluations().words());
    const RqNTTVec h = vp.sum();
    EXPECT(h.words() == sum_of_terms(cfg, whole, terms, coeffs, full));
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
        const RqNTTVec msg = vp.round_evals(order);
        EXPECT(msg.len() == degree + 1);
        Words t(w, 0);  // t * one
        for (size_t pt = 0; pt <= degree; pt++) {
            std::vector<Words> folded;
            for (const Mle &m : mles)
                folded.push_back(order == SR_MLE_LEADING ? m.fixed_variables(RqNTTVec(cfg, t)).words() : m.fix_last_variables(RqNTTVec(cfg, t)).words());
            const Words want = sum_of_terms(cfg, folded, terms, coeffs, full / 2);
            EXPECT(Words(msg.words().begin() + pt * w, msg.words().begin() + (pt + 1) * w) == want);
            CyclotomicConfig::check(sr_add_batch(cfg.raw(), t.data(), one.words().data(), 1), "add");
        }
        // p(0) + p(1) is the claimed sum
        Words s(msg.words().begin(), msg.words().begin() + w);
        CyclotomicConfig::check(sr_add_batch(cfg.raw(), s.data(), msg.words().data() + w, 1), "add");
        EXPECT(s == h.words());
    }
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t full = (size_t)1 << nv;
    structure(cfg, field, nv, {{0, 1, 2}, {0, 3}}, 4, 0x7C00);            // R1CS
    structure(cfg, field, nv, {{0, 0, 1, 1}, {1}, {2, 3}}, 4, 0x7D00);    // REPEAT
    // eq (a b - c) built the way HyperPlonk builds it, without coefficients where they are one(): one product of three and the message
    // of DenseMultilinearExtension::round_evals
    Mle e(cfg, nv, uniform(field, 1, full * cfg.dimension())), a(cfg, nv, uniform(field, 2, (full - 1) * cfg.dimension()));
    Mle b(cfg, nv, uniform(field, 3, full * cfg.dimension())), shorter(cfg, nv - 1, uniform(field, 4, (full / 2) * cfg.dimension()));
    VirtualPolynomial single(cfg, nv);
    single.add_mle_list({&a, &b});
    single.mul_by_mle(&e);
    EXPECT(single.degree() == 3 && single.tables().size() == 3);
    EXPECT(single.round_evals().words() == Mle::round_evals({&a, &b, &e}).words());
    EXPECT(single.sum().words() == Mle::product_sum({&a, &b, &e}).words());
    // the limits throw and leave the polynomial as it was
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    std::vector<Mle> many;
    for (int j = 0; j < 9; j++) many.emplace_back(cfg, nv, uniform(field, 16 + j, cfg.dimension()));
    VirtualPolynomial v8(cfg, nv);
    for (int j = 0; j < 4; j++) v8.add_mle_list({&many[2 * j], &many[2 * j + 1]});
    EXPECT(throws([&] { v8.add_mle_list({&many[0], &many[8]}); }));  // the ninth table
    EXPECT(v8.tables().size() == 8 && v8.terms().size() == 4);
    for (int j = 0; j < 4; j++) v8.add_mle_list({&many[j]});
    EXPECT(throws([&] { v8.add_mle_list({&many[0]}); }));  // the ninth product
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).add_mle_list({&e, &e, &e, &e, &e}); }));  // the fifth factor
    VirtualPolynomial v4(cfg, nv);
    v4.add_mle_list({&e, &a, &b, &e});
    EXPECT(throws([&] { v4.mul_by_mle(&a); }));
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).add_mle_list({&e, &shorter}); }));
    EXPECT(throws([&] { VirtualPolynomial(cfg, nv).round_evals(); }));
    EXPECT(throws([&] { single.round_evals(2); }));
    std::printf("%s ok\n", name);
}

int main() {
    family("goldilocks", SR_RING_GOLDILOCKS_POW2, SRO_GOLDILOCKS, 6, 7);
    family("babybear", SR_RING_BABYBEAR_POW2, SRO_BABYBEAR, 5, 6);
    family("stark", SR_RING_STARK_POW2, SRO_STARK, 4, 6);
    family("goldilocks24", SR_RING_GOLDILOCKS_24, SRO_GOLDILOCKS, 0, 7);
    family("babybear72", SR_RING_BABYBEAR_72, SRO_BABYBEAR, 0, 6);
    family("frog16", SR_RING_FROG_16, SRO_FROG, 0, 7);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
