// DenseMultilinearExtension::fold_round_evals of include/stark_rings.hpp against the two calls it merges: fixed_variables /
// fix_last_variables of every table at r, then round_evals of the folded tables -- one shape per ring family, both orders, truncated
// tables of different lengths, bit for bit; and the throws where the C call refuses.
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

static void family(const char *name, sr_ring ring, int field, int log2d, size_t nv) {
    CyclotomicConfig cfg(ring, log2d);
    const size_t w = cfg.words_per_elem(), full = (size_t)1 << nv, half = full / 2;
    const RqNTTVec r(cfg, uniform(field, 0xF01D, cfg.dimension()));
    for (size_t d = 1; d <= 4; d++) {
        std::vector<Mle> mles;
        for (size_t j = 0; j < d; j++) {
            const size_t n = j == 1 ? full - 3 : j == 2 ? half + 1 : full;  // truncated tables of different lengths
            mles.emplace_back(cfg, nv, uniform(field, 0xF0 + 16 * d + j, n * cfg.dimension()));
        }
        std::vector<const Mle *> ptrs;
        for (const Mle &m : mles) ptrs.push_back(&m);
        for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING}) {
            auto got = Mle::fold_round_evals(ptrs, r, order);
            EXPECT(got.first.len() == d + 1 && got.second.size() == d);
            std::vector<Mle> folded;
            for (const Mle &m : mles) folded.push_back(order == SR_MLE_LEADING ? m.fixed_variables(r) : m.fix_last_variables(r));
            std::vector<const Mle *> fp;
            for (const Mle &m : folded) fp.push_back(&m);
            EXPECT(got.first.words() == Mle::round_evals(fp, order).words());
            for (size_t j = 0; j < d; j++) {
                const size_t n = mles[j].len(), n_out = order == SR_MLE_LEADING ? (n + 1) / 2 : (n < half ? n : half);
                EXPECT(got.second[j].num_vars() == nv - 1 && got.second[j].len() == n_out);
                EXPECT(got.second[j].words() == Words(folded[j].words().begin(), folded[j].words().begin() + n_out * w));
                EXPECT(got.second[j].to_evaluations().words() == folded[j].words());  // the rest of the folded table is zero
            }
        }
    }
    // the refusals throw
    Mle a(cfg, nv, uniform(field, 1, full * cfg.dimension())), shorter(cfg, nv - 1, uniform(field, 2, half * cfg.dimension()));
    Mle one_var(cfg, 1, uniform(field, 3, 2 * cfg.dimension()));
    auto throws = [](auto fn) {
        try {
            fn();
        } catch (const std::exception &) {
            return true;
        }
        return false;
    };
    EXPECT(throws([&] { Mle::fold_round_evals({}, r); }));
    EXPECT(throws([&] { Mle::fold_round_evals({&a, &a, &a, &a, &a}, r); }));
    EXPECT(throws([&] { Mle::fold_round_evals({&a, &shorter}, r); }));
    EXPECT(throws([&] { Mle::fold_round_evals({&a}, r, 2); }));
    EXPECT(throws([&] { Mle::fold_round_evals({&one_var}, r); }));  // the folded table needs a variable for the next round
    EXPECT(throws([&] { Mle::fold_round_evals({&a}, RqNTTVec(cfg, uniform(field, 4, 2 * cfg.dimension()))); }));
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
