// DenseMultilinearExtension::round_evals / product_sum of include/stark_rings.hpp against the composition of the mirror's older
// calls: every table folded at the point [t * one] (fixed_variables / fix_last_variables; one() is eq_table of the empty point), the
// folded tables multiplied slot-wise (sr_pointwise_mul_batch) and summed (sr_sum_batch) -- one shape per ring family, both orders, a
// truncated table, bit for bit; and the throws where the C call refuses.
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

// sum_b prod_j tables[j][b] from the older calls; every table holds all `n` elements
static Words sum_of_products(const CyclotomicConfig &cfg, const std::vector<Words> &tables, size_t n) {
    Words acc = tables[0];
    for (size_t j = 1; j < tables.size(); j++) CyclotomicConfig::check(sr_pointwise_mul_batch(cfg.raw(), acc.data(), tables[j].data(), n), "pointwise");
    Words out(cfg.words_per_elem());
    CyclotomicConfig::check(sr_sum_batch(cfg.raw(), out.data(), acc.data(), n), "sum");
    return out;
}

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t w = cfg.words_per_elem(), full = (size_t)1 << nv;
    const RqNTTVec one = eq_table(RqNTTVec(cfg, Words()));
    for (size_t d = 1; d <= 4; d++) {
        std::vector<Mle> mles;
        for (size_t j = 0; j < d; j++) {
            const size_t n = j == 1 ? full - 3 : full;  // one truncated table
            mles.emplace_back(cfg, nv, uniform(field, 0x5C0 + 16 * d + j, n * cfg.dimension()));
        }
        std::vector<const Mle *> ptrs;
        for (const Mle &m : mles) ptrs.push_back(&m);
        std::vector<Words> whole;
        for (const Mle &m : mles) whole.push_back(m.to_evaluations().words());
        const RqNTTVec h = Mle::product_sum(ptrs);
        EXPECT(h.words() == sum_of_products(cfg, whole, full));
        for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
            const RqNTTVec msg = Mle::round_evals(ptrs, order);
            EXPECT(msg.len() == d + 1);
            Words t(w, 0);  // t * one
            for (size_t pt = 0; pt <= d; pt++) {
                std::vector<Words> folded;
                for (const Mle &m : mles)
                    folded.push_back(order == SR_MLE_LEADING ? m.fixed_variables(RqNTTVec(cfg, t)).words() : m.fix_last_variables(RqNTTVec(cfg, t)).words());
                const Words want = sum_of_products(cfg, folded, full / 2);
                EXPECT(Words(msg.words().begin() + pt * w, msg.words().begin() + (pt + 1) * w) == want);
                CyclotomicConfig::check(sr_add_batch(cfg.raw(), t.data(), one.words().data(), 1), "add");
            }
            // p(0) + p(1) is the claimed sum
            Words s(msg.words().begin(), msg.words().begin() + w);
            CyclotomicConfig::check(sr_add_batch(cfg.raw(), s.data(), msg.words().data() + w, 1), "add");
            EXPECT(s == h.words());
        }
        if (d == 2) {  // the same table twice
            std::vector<const Mle *> twice = {&mles[0], &mles[0]};
            EXPECT(Mle::product_sum(twice).words() == sum_of_products(cfg, {whole[0], whole[0]}, full));
        }
    }
    // the refusals throw
    Mle a(cfg, nv, uniform(field, 1, full * cfg.dimension())), shorter(cfg, nv - 1, uniform(field, 2, (full / 2) * cfg.dimension()));
    Mle none(cfg, 0, uniform(field, 3, cfg.dimension()));
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    EXPECT(throws([&] { Mle::round_evals({}); }));
    EXPECT(throws([&] { Mle::round_evals({&a, &a, &a, &a, &a}); }));
    EXPECT(throws([&] { Mle::round_evals({&a, &shorter}); }));
    EXPECT(throws([&] { Mle::round_evals({&a}, 2); }));
    EXPECT(throws([&] { Mle::round_evals({&none}); }));  // a round needs a variable
    EXPECT(Mle::product_sum({&none}).words() == none.words());
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
