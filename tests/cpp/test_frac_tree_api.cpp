// FractionTree, frac_tree and frac_tree_plan of include/stark_rings.hpp against a pair-at-a-time restatement of the fraction tree
// whose products come from the oracle (libsr_oracle) and whose sums are limb arithmetic modulo the base prime on the memory image (the
// Montgomery form is linear): one tree per ring family, both orders, full and truncated leaves, with and without stored numerators,
// bit for bit; the q side against ProductTree.
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
    Words prime;  // little-endian limbs
};

// a <- a + b mod p on `limbs` little-endian words, a and b below p
static void add_mod(uint64_t *a, const uint64_t *b, const Words &p) {
    const size_t n = p.size();
    unsigned carry = 0;
    for (size_t i = 0; i < n; i++) {
        const unsigned __int128 s = (unsigned __int128)a[i] + b[i] + carry;
        a[i] = (uint64_t)s;
        carry = (unsigned)(s >> 64);
    }
    bool ge = carry != 0;
    if (!ge) {
        ge = true;
        for (size_t i = n; i-- > 0;)
            if (a[i] != p[i]) {
                ge = a[i] > p[i];
                break;
            }
    }
    if (ge) {
        unsigned borrow = 0;
        for (size_t i = 0; i < n; i++) {
            const unsigned __int128 d = (unsigned __int128)a[i] - p[i] - borrow;
            a[i] = (uint64_t)d;
            borrow = (unsigned)((d >> 64) & 1);
        }
    }
}

// layers 1 .. nv of both sides, one behind the other; `p` and `q` hold all 2^nv leaves
static void restate(const Family &f, Words p, Words q, size_t nv, int order, size_t w, Words *p_out, Words *q_out) {
    const size_t limbs = f.prime.size();
    for (size_t k = 1; k <= nv; k++) {
        const size_t half = (size_t)1 << (nv - k);
        Words np(half * w), nq(half * w), t(w);
        for (size_t i = 0; i < half; i++) {
            const size_t l = (order == SR_MLE_LEADING ? 2 * i : i) * w, r = (order == SR_MLE_LEADING ? 2 * i + 1 : i + half) * w;
            std::copy(p.begin() + l, p.begin() + l + w, np.begin() + i * w);
            f.mul(np.data() + i * w, q.data() + r);   // p_l q_r
            std::copy(p.begin() + r, p.begin() + r + w, t.begin());
            f.mul(t.data(), q.data() + l);            // p_r q_l
            for (size_t c = 0; c < w; c += limbs) add_mod(np.data() + i * w + c, t.data() + c, f.prime);
            std::copy(q.begin() + l, q.begin() + l + w, nq.begin() + i * w);
            f.mul(nq.data() + i * w, q.data() + r);
        }
        p_out->insert(p_out->end(), np.begin(), np.end());
        q_out->insert(q_out->end(), nq.begin(), nq.end());
        p.swap(np);
        q.swap(nq);
    }
}

static void family_suite(const Family &f, size_t nv) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const int limbs = sro_limbs(f.field);
    const size_t w = cfg.words_per_elem(), full = (size_t)1 << nv;
    Words p_all(full * w), q_all(full * w);
    sro_fill_uniform(f.field, 0xE0 + nv, 0, full * f.degree, p_all.data());
    sro_fill_uniform(f.field, 0xF0 + nv, 0, full * f.degree, q_all.data());
    Words one(w, 0), m1(limbs), std1(limbs, 0);
    std1[0] = 1;
    sro_to_mont(f.field, std1.data(), m1.data(), 1);
    for (size_t i = 0; i < f.degree; i += f.slot_w) std::copy(m1.begin(), m1.end(), one.begin() + i * limbs);
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING})
        for (size_t n_leaves : {full, full - 3, (size_t)5, (size_t)0})
            for (bool has_p : {true, false}) {
                const Words ps(p_all.begin(), p_all.begin() + n_leaves * w), qs(q_all.begin(), q_all.begin() + n_leaves * w);
                Words pp, qp(qs);
                for (size_t e = 0; e < n_leaves; e++)
                    if (has_p) pp.insert(pp.end(), ps.begin() + e * w, ps.begin() + (e + 1) * w);
                    else pp.insert(pp.end(), one.begin(), one.end());
                pp.resize(full * w, 0);
                for (size_t e = n_leaves; e < full; e++) qp.insert(qp.end(), one.begin(), one.end());
                Words want_p, want_q;
                restate(f, pp, qp, nv, order, w, &want_p, &want_q);
                const FractionTree tree = has_p ? FractionTree(cfg, ps, qs, nv, order) : FractionTree(cfg, qs, nv, order);
                EXPECT(tree.num_vars() == nv && tree.n_leaves() == n_leaves && tree.order() == order && tree.has_numerators() == has_p);
                EXPECT(tree.p_layer_words() == want_p);
                EXPECT(tree.q_layer_words() == want_q);
                if (tree.p_layer_words() != want_p || tree.q_layer_words() != want_q)
                    std::printf("  %s order %d n_leaves %zu numerators %d\n", f.name, order, n_leaves, (int)has_p);
                EXPECT(tree.q_layer_words() == ProductTree(cfg, qs, nv, order).layer_words());
                const auto both = frac_tree(cfg, has_p ? &ps : nullptr, qs, nv, order);
                EXPECT(both.first == want_p && both.second == want_q);
                const auto root = tree.root();
                EXPECT(root.first.words() == Words(want_p.end() - w, want_p.end()) && root.second.words() == Words(want_q.end() - w, want_q.end()));
                size_t end = 0;
                for (size_t k = 1; k <= nv; k++) {
                    EXPECT(tree.layer_offset(k) == end);
                    const auto lk = tree.layer(k);
                    const size_t len = (size_t)1 << (nv - k);
                    EXPECT(lk.first.num_vars() == nv - k && lk.second.num_vars() == nv - k && lk.first.len() == len && lk.second.len() == len);
                    EXPECT(lk.first.words() == Words(want_p.begin() + end * w, want_p.begin() + (end + len) * w));
                    EXPECT(lk.second.words() == Words(want_q.begin() + end * w, want_q.begin() + (end + len) * w));
                    end += len;
                    if (order == SR_MLE_TRAILING && (k > 1 || (n_leaves == full && has_p))) {
                        const auto h = tree.halves(k);
                        EXPECT(h.size() == 4 && h[0].num_vars() == nv - k && h[3].len() == len);
                        const RqNTTVec p_lo(cfg, h[0].words()), p_hi(cfg, h[1].words()), q_lo(cfg, h[2].words()), q_hi(cfg, h[3].words());
                        EXPECT((q_lo * q_hi).words() == lk.second.words());
                        Words sum = (p_lo * q_hi).words();
                        const Words other = (p_hi * q_lo).words();
                        for (size_t c = 0; c < sum.size(); c += limbs) add_mod(sum.data() + c, other.data() + c, f.prime);
                        EXPECT(sum == lk.first.words());
                    }
                }
                if (order == SR_MLE_LEADING) EXPECT_THROWS(tree.halves(1));
                if (n_leaves != full || !has_p) EXPECT_THROWS(tree.layer(0));
                else EXPECT(tree.layer(0).first.words() == ps && tree.layer(0).second.words() == qs);
                EXPECT_THROWS(tree.layer(nv + 1));
                EXPECT_THROWS(tree.layer_offset(0));
            }
    EXPECT_THROWS(FractionTree(cfg, p_all, q_all, nv - 1, SR_MLE_TRAILING));                            // more leaves than 2^num_vars
    EXPECT_THROWS(FractionTree(cfg, p_all, q_all, nv, 2));                                              // unknown order
    EXPECT_THROWS(FractionTree(cfg, Words(p_all.begin(), p_all.begin() + w), q_all, nv));               // numerators of another length
    const Words p0(p_all.begin(), p_all.begin() + w), q0(q_all.begin(), q_all.begin() + w);
    const FractionTree single(cfg, p0, q0, 0);
    EXPECT(single.p_layer_words().empty() && single.q_layer_words().empty());
    EXPECT(single.root().first.words() == p0 && single.root().second.words() == q0);
    EXPECT_THROWS(FractionTree(cfg, q0, 0).root());
    const auto plan = FractionTree::plan(f.ring, f.log2d, nv);
    EXPECT(plan.first == full - 1 && plan.second >= 2 && plan.second <= (int)nv);
    EXPECT(frac_tree_plan(f.ring, f.log2d, 0).second == 0);
    std::printf("%s: done\n", f.name);
}

int main() {
    auto pow2 = [](int field, size_t d) { return [field, d](uint64_t *l, const uint64_t *r) { sro_pow2_pointwise(field, l, r, d); }; };
    const Words gl = {0xFFFFFFFF00000001ull}, bb = {2013265921ull}, frog = {15912092521325583641ull},
                stark = {1ull, 0ull, 0ull, 0x0800000000000011ull};
    const Family fams[] = {
        {"goldilocks 2^6", SR_RING_GOLDILOCKS_POW2, 0, 6, 64, 1, pow2(0, 64), gl},
        {"babybear 2^5", SR_RING_BABYBEAR_POW2, 1, 5, 32, 1, pow2(1, 32), bb},
        {"stark 2^4", SR_RING_STARK_POW2, 2, 4, 16, 1, pow2(2, 16), stark},
        {"goldilocks24", SR_RING_GOLDILOCKS_24, 0, 0, 24, 3, sro_g24_ntt_mul, gl},
        {"babybear72", SR_RING_BABYBEAR_72, 1, 0, 72, 9, sro_bb72_ntt_mul, bb},
        {"frog16", SR_RING_FROG_16, 3, 0, 16, 4, sro_frog16_ntt_mul, frog},
    };
    for (const Family &f : fams) family_suite(f, 5);
    std::printf(failures ? "frac tree api: %d FAILURES\n" : "frac tree api: all ok\n", failures);
    return failures ? 1 : 0;
}
