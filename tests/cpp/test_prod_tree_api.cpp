// ProductTree of include/stark_rings.hpp against a pair-at-a-time restatement of the layered grand product whose products come from
// the oracle (libsr_oracle): one tree per ring family, both orders, full and truncated leaves, bit for bit; the root against
// RqNTTVec::product and, in trailing order, every layer against the element-wise product of halves().
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../include/stark_rings.hpp"
#include "../../oracle/sr_oracle.h"

using namespace stark_rings;
typedef std::vector<uint64_t> Words;

static int failures = 0;
#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond);    \
            failures++;                                                    \
        }                                                                  \
    } while (0)
#define EXPECT_THROWS(expr)                                                \
    do {                                                                   \
        bool threw = false;                                                \
        try { (void)(expr); } catch (const std::exception &) { threw = true; } \
        EXPECT(threw);                                                     \
    } while (0)

struct Family {
    const char *name;
    sr_ring ring;
    int field, log2d;
    size_t degree, slot_w;  // slot_w: coefficients per slot (component 0 of every slot of one() is 1)
    std::function<void(uint64_t *, const uint64_t *)> mul;  // lhs <- lhs * rhs, one ring element, slot-wise
};

// layers 1 .. nv, one behind the other; `leaves` holds all 2^nv elements
static Words restate(const Family &f, Words below, size_t nv, int order, size_t w) {
    Words out;
    for (size_t k = 1; k <= nv; k++) {
        const size_t half = (size_t)1 << (nv - k);
        Words next(half * w);
        for (size_t i = 0; i < half; i++) {
            const uint64_t *lo = below.data() + (order == SR_MLE_LEADING ? 2 * i : i) * w;
            const uint64_t *hi = below.data() + (order == SR_MLE_LEADING ? 2 * i + 1 : i + half) * w;
            std::copy(lo, lo + w, next.begin() + i * w);
            f.mul(next.data() + i * w, hi);
        }
        out.insert(out.end(), next.begin(), next.end());
        below.swap(next);
    }
    return out;
}

static void family_suite(const Family &f, size_t nv) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const int limbs = sro_limbs(f.field);
    const size_t w = cfg.words_per_elem(), full = (size_t)1 << nv;
    Words leaves(full * w);
    sro_fill_uniform(f.field, 0xD0 + nv, 0, full * f.degree, leaves.data());
    Words one(w, 0), m1(limbs), std1(limbs, 0);
    std1[0] = 1;
    sro_to_mont(f.field, std1.data(), m1.data(), 1);
    for (size_t i = 0; i < f.degree; i += f.slot_w) std::copy(m1.begin(), m1.end(), one.begin() + i * limbs);
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING})
        for (size_t n_leaves : {full, full - 3, (size_t)5, (size_t)0}) {
            Words stored(leaves.begin(), leaves.begin() + n_leaves * w), padded(stored);
            for (size_t e = n_leaves; e < full; e++) padded.insert(padded.end(), one.begin(), one.end());
            const Words want = restate(f, padded, nv, order, w);
            const ProductTree tree(cfg, stored, nv, order);
            EXPECT(tree.num_vars() == nv && tree.n_leaves() == n_leaves && tree.order() == order);
            EXPECT(tree.layer_words() == want);
            if (tree.layer_words() != want) std::printf("  %s order %d n_leaves %zu\n", f.name, order, n_leaves);
            EXPECT(tree.root().words() == Words(want.end() - w, want.end()));
            EXPECT(tree.root().words() == RqNTTVec(cfg, stored).product().words());
            size_t end = 0;
            for (size_t k = 1; k <= nv; k++) {
                EXPECT(tree.layer_offset(k) == end);
                const DenseMultilinearExtension lk = tree.layer(k);
                EXPECT(lk.num_vars() == nv - k && lk.len() == (size_t)1 << (nv - k));
                EXPECT(lk.words() == Words(want.begin() + end * w, want.begin() + (end + lk.len()) * w));
                end += lk.len();
                if (order == SR_MLE_TRAILING && (k > 1 || n_leaves == full)) {
                    const auto h = tree.halves(k);
                    EXPECT(h.first.num_vars() == nv - k && h.second.num_vars() == nv - k);
                    EXPECT((RqNTTVec(cfg, h.first.words()) * RqNTTVec(cfg, h.second.words())).words() == lk.words());
                }
            }
            if (order == SR_MLE_LEADING) EXPECT_THROWS(tree.halves(1));
            if (n_leaves != full) EXPECT_THROWS(tree.layer(0));
            else EXPECT(tree.layer(0).words() == stored);
            EXPECT_THROWS(tree.layer(nv + 1));
            EXPECT_THROWS(tree.layer_offset(0));
        }
    EXPECT_THROWS(ProductTree(cfg, leaves, nv - 1, SR_MLE_TRAILING));   // more leaves than 2^num_vars
    EXPECT_THROWS(ProductTree(cfg, leaves, nv, 2));                     // unknown order
    const ProductTree single(cfg, Words(leaves.begin(), leaves.begin() + w), 0);
    EXPECT(single.layer_words().empty() && single.root().words() == Words(leaves.begin(), leaves.begin() + w));
    const auto plan = ProductTree::plan(f.ring, f.log2d, nv);
    EXPECT(plan.first == full - 1 && plan.second >= 2 && plan.second <= (int)nv);
    std::printf("%s: done\n", f.name);
}

int main() {
    auto pow2 = [](int field, size_t d) { return [field, d](uint64_t *l, const uint64_t *r) { sro_pow2_pointwise(field, l, r, d); }; };
    const Family fams[] = {
        {"goldilocks 2^6", SR_RING_GOLDILOCKS_POW2, 0, 6, 64, 1, pow2(0, 64)},
        {"babybear 2^5", SR_RING_BABYBEAR_POW2, 1, 5, 32, 1, pow2(1, 32)},
        {"stark 2^4", SR_RING_STARK_POW2, 2, 4, 16, 1, pow2(2, 16)},
        {"goldilocks24", SR_RING_GOLDILOCKS_24, 0, 0, 24, 3, sro_g24_ntt_mul},
        {"babybear72", SR_RING_BABYBEAR_72, 1, 0, 72, 9, sro_bb72_ntt_mul},
        {"frog16", SR_RING_FROG_16, 3, 0, 16, 4, sro_frog16_ntt_mul},
    };
    for (const Family &f : fams) family_suite(f, 5);
    std::printf(failures ? "prod tree api: %d FAILURES\n" : "prod tree api: all ok\n", failures);
    return failures ? 1 : 0;
}
