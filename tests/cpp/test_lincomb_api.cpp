// lincomb, lincomb_plan, DenseMultilinearExtension::linear_combination, permutation_leaves, fingerprint, PermutationCheck and
// LookupCheck of include/stark_rings.hpp against a term-at-a-time restatement whose products come from the oracle (libsr_oracle) and
// whose sums are limb arithmetic modulo the base prime on the memory image (the Montgomery form is linear): one ring per family, both
// kernels, masked rows, truncated tables, bit for bit; one permutation check and one lookup check.
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
// a <- p - a (a below p; zero stays zero)
static void neg_mod(uint64_t *a, const Words &p) {
    bool zero = true;
    for (size_t i = 0; i < p.size(); i++) zero = zero && a[i] == 0;
    if (zero) return;
    unsigned borrow = 0;
    for (size_t i = 0; i < p.size(); i++) {
        const unsigned __int128 d = (unsigned __int128)p[i] - a[i] - borrow;
        a[i] = (uint64_t)d;
        borrow = (unsigned)((d >> 64) & 1);
    }
}

// one term at a time: out_m[e] = [bit K] c_m[K] + sum_k [bit k] c_m[k] * T_k[e]
static std::vector<Words> restate(const Family &f, const std::vector<Words> &tables, const Words &coef, const std::vector<uint32_t> &uses, size_t n,
                                  size_t w) {
    const size_t limbs = f.prime.size(), K = tables.size();
    std::vector<Words> outs;
    for (size_t m = 0; m < uses.size(); m++) {
        Words out(n * w, 0), t(w);
        for (size_t e = 0; e < n; e++) {
            for (size_t k = 0; k < K; k++) {
                if (!((uses[m] >> k) & 1) || (e + 1) * w > tables[k].size()) continue;
                std::copy(tables[k].begin() + e * w, tables[k].begin() + (e + 1) * w, t.begin());
                f.mul(t.data(), coef.data() + (m * (K + 1) + k) * w);
                for (size_t c = 0; c < w; c += limbs) add_mod(out.data() + e * w + c, t.data() + c, f.prime);
            }
            if ((uses[m] >> K) & 1)
                for (size_t c = 0; c < w; c += limbs) add_mod(out.data() + e * w + c, coef.data() + (m * (K + 1) + K) * w + c, f.prime);
        }
        outs.push_back(out);
    }
    return outs;
}

static Words uniform(const Family &f, uint64_t seed, size_t n_elems, size_t w) {
    Words out(n_elems * w);
    sro_fill_uniform(f.field, seed, 0, n_elems * f.degree, out.data());
    return out;
}
static Words slice(const Words &v, size_t a, size_t b, size_t w) { return Words(v.begin() + a * w, v.begin() + b * w); }

static void family_suite(const Family &f) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const int limbs = sro_limbs(f.field);
    const size_t w = cfg.words_per_elem(), n = 9;
    Words one(w, 0), m1(limbs), std1(limbs, 0);
    std1[0] = 1;
    sro_to_mont(f.field, std1.data(), m1.data(), 1);
    for (size_t i = 0; i < f.degree; i += f.slot_w) std::copy(m1.begin(), m1.end(), one.begin() + i * limbs);
    // both kernels (K = 3 / 5), several launches (M = 4), masks, truncation
    for (size_t K : {(size_t)1, (size_t)3, (size_t)5, (size_t)16})
        for (size_t M : {(size_t)1, (size_t)2, (size_t)4}) {
            std::vector<Words> tables;
            for (size_t k = 0; k < K; k++) tables.push_back(uniform(f, 0x100 * K + k, k % 3 == 1 ? n - 1 : (k == 4 ? 0 : n), w));
            const Words coef = uniform(f, 0x7000 + 16 * K + M, M * (K + 1), w);
            std::vector<uint32_t> uses(M, ((uint32_t)2 << K) - 1);
            if (M > 1 && K > 1) uses[1] = (((uint32_t)1 << K) - 1) & ~2u;   // no table 1, no constant
            std::vector<const Words *> ptrs;
            for (const Words &t : tables) ptrs.push_back(&t);
            const auto got = lincomb(cfg, ptrs, coef, uses, n);
            const auto want = restate(f, tables, coef, uses, n, w);
            EXPECT(got == want);
            if (got != want) std::printf("  %s K %zu M %zu\n", f.name, K, M);
            const auto plan = lincomb_plan(f.ring, f.log2d, (int)K, (int)M);
            EXPECT(plan.first * plan.second >= (int)M && plan.second >= 1 && plan.second <= (int)M);
        }
    {   // the class: three truncated MLEs in three variables, with and without the constant
        std::vector<DenseMultilinearExtension> mles;
        std::vector<Words> tables;
        for (size_t k = 0; k < 3; k++) {
            tables.push_back(uniform(f, 0x300 + k, k == 1 ? 0 : 5 + k, w));
            mles.emplace_back(cfg, 3, tables.back());
        }
        const Words cw = uniform(f, 0x310, 4, w);
        const RqNTTVec coeffs(cfg, slice(cw, 0, 3, w)), constant(cfg, slice(cw, 3, 4, w));
        const auto a = DenseMultilinearExtension::linear_combination({&mles[0], &mles[1], &mles[2]}, coeffs);
        EXPECT(a.num_vars() == 3 && a.len() == 7 && a.words() == restate(f, tables, cw, {0x7u}, 7, w)[0]);
        const auto b = DenseMultilinearExtension::linear_combination({&mles[0], &mles[1], &mles[2]}, coeffs, &constant);
        EXPECT(b.len() == 8 && b.words() == restate(f, tables, cw, {0xFu}, 8, w)[0]);
        EXPECT_THROWS(DenseMultilinearExtension::linear_combination({&mles[0], &mles[1]}, coeffs));
        EXPECT_THROWS(DenseMultilinearExtension::linear_combination({}, coeffs));
    }
    {   // refusals of the host form
        const Words t = uniform(f, 0x400, n, w), coef = uniform(f, 0x401, 3, w);
        EXPECT_THROWS(lincomb(cfg, {&t, &t}, coef, {0x0u}, n));      // an empty mask
        EXPECT_THROWS(lincomb(cfg, {&t, &t}, coef, {0x8u}, n));      // a bit above n_tables
        EXPECT_THROWS(lincomb(cfg, {&t, &t}, coef, {0x5u}, n));      // table 1 unused
        EXPECT_THROWS(lincomb(cfg, {&t, &t}, coef, {0x7u}, n - 1));  // n_evals > n
        EXPECT_THROWS(lincomb(cfg, {&t}, coef, {0x3u}, n));          // coef of the wrong size
        EXPECT_THROWS(lincomb_plan(f.ring, f.log2d, 17, 1));
        EXPECT_THROWS(lincomb_plan(f.ring, f.log2d, 1, 5));
        const Words none;
        EXPECT(lincomb(cfg, {&none, &none}, coef, {0x7u}, 0)[0].empty());   // n = 0: nothing launched, nothing written
    }
    {   // a permutation check: two columns of 2^3 rows, sigma a rotation of the 16 positions, every wire value the same
        const size_t rows = 8, total = 16;
        const Words ident = uniform(f, 0x500, total, w), value = uniform(f, 0x501, 1, w);
        const RqNTTVec beta(cfg, uniform(f, 0x502, 1, w)), gamma(cfg, uniform(f, 0x503, 1, w)), one_v(cfg, one);
        Words fw, sigma;
        for (size_t i = 0; i < total; i++) {
            fw.insert(fw.end(), value.begin(), value.end());
            const size_t j = (i + 5) % total;
            sigma.insert(sigma.end(), ident.begin() + j * w, ident.begin() + (j + 1) * w);
        }
        auto build = [&](const Words &sg) {
            Words num, den;
            for (size_t c = 0; c < 2; c++) {
                const auto nd = permutation_leaves(cfg, slice(fw, c * rows, (c + 1) * rows, w), slice(ident, c * rows, (c + 1) * rows, w),
                                                   slice(sg, c * rows, (c + 1) * rows, w), beta, gamma, one_v);
                num.insert(num.end(), nd.first.begin(), nd.first.end());
                den.insert(den.end(), nd.second.begin(), nd.second.end());
            }
            return PermutationCheck(cfg, num, den, 4);
        };
        const PermutationCheck ok = build(sigma);
        EXPECT(ok.holds() && ok.roots().first.words() == ok.roots().second.words());
        // the numerator leaves against the restatement: tables (f, id, sigma), row (one, gamma, -, beta)
        Words coef(one);
        for (const RqNTTVec *c : {&gamma, &gamma, &beta}) coef.insert(coef.end(), c->words().begin(), c->words().end());
        const auto want = restate(f, {slice(fw, 0, rows, w), slice(ident, 0, rows, w), slice(sigma, 0, rows, w)}, coef, {0xBu}, rows, w);
        Words all(want[0]);
        const auto second = restate(f, {slice(fw, rows, total, w), slice(ident, rows, total, w), slice(sigma, rows, total, w)}, coef, {0xBu}, rows, w);
        all.insert(all.end(), second[0].begin(), second[0].end());
        EXPECT(ok.num().layer(0).words() == all);
        Words bad(sigma);
        std::copy(ident.begin(), ident.begin() + w, bad.begin() + 3 * w);   // position 3 now points at 0 instead of 8
        EXPECT(!build(bad).holds());
        const RqNTTVec z(cfg, uniform(f, 0x504, 3, w));
        auto claim = ok.layer_claim(0, 1, z);
        const RqNTTVec msg = claim->sumcheck().message();
        RqNTTVec sum(cfg, slice(msg.words(), 0, 1, w));
        sum += RqNTTVec(cfg, slice(msg.words(), 1, 2, w));
        EXPECT(sum.words() == ok.num().layer(1).evaluate(z)->words());
    }
    {   // a lookup check: 2^3 witness rows from a 2^2-row table of two columns, q = beta - (c_0 + gamma c_1)
        const Words c0 = uniform(f, 0x600, 4, w), c1 = uniform(f, 0x601, 4, w), gm = uniform(f, 0x602, 1, w);
        const size_t picks[8] = {0, 2, 2, 3, 0, 2, 3, 2};
        size_t mult[4] = {0, 0, 0, 0};
        Words w0, w1;
        for (size_t i : picks) {
            mult[i]++;
            w0.insert(w0.end(), c0.begin() + i * w, c0.begin() + (i + 1) * w);
            w1.insert(w1.end(), c1.begin() + i * w, c1.begin() + (i + 1) * w);
        }
        Words minus_one(one), minus_gamma(gm);
        for (size_t c = 0; c < w; c += limbs) {
            neg_mod(minus_one.data() + c, f.prime);
            neg_mod(minus_gamma.data() + c, f.prime);
        }
        Words cw(minus_one);
        cw.insert(cw.end(), minus_gamma.begin(), minus_gamma.end());
        const RqNTTVec coeffs(cfg, cw);
        auto mults = [&](const size_t *m) {
            Words out;
            for (size_t j = 0; j < 4; j++) {
                Words e(w, 0);
                for (size_t r = 0; r < m[j]; r++)
                    for (size_t c = 0; c < w; c += limbs) add_mod(e.data() + c, one.data() + c, f.prime);
                out.insert(out.end(), e.begin(), e.end());
            }
            return out;
        };
        auto build = [&](const Words &beta_w, const size_t *m) {
            const RqNTTVec beta(cfg, beta_w);
            return LookupCheck(cfg, fingerprint(cfg, {&w0, &w1}, coeffs, &beta), fingerprint(cfg, {&c0, &c1}, coeffs, &beta), mults(m), 3, 2);
        };
        const Words beta_w = uniform(f, 0x603, 1, w);
        EXPECT(build(beta_w, mult).holds());
        Words full(cw);
        full.insert(full.end(), beta_w.begin(), beta_w.end());
        const RqNTTVec beta_v(cfg, beta_w);
        const Words q_t = fingerprint(cfg, {&c0, &c1}, coeffs, &beta_v);
        EXPECT(q_t == restate(f, {c0, c1}, full, {0x7u}, 4, w)[0]);
        // beta equal to the fingerprint of table row 2: a zero denominator, and the identity still holds
        Words at_row = slice(c1, 2, 3, w);
        f.mul(at_row.data(), gm.data());
        for (size_t c = 0; c < w; c += limbs) add_mod(at_row.data() + c, c0.data() + 2 * w + c, f.prime);
        const LookupCheck zero_den = build(at_row, mult);
        EXPECT(zero_den.table().layer(0).second.words().size() == 4 * w);
        EXPECT(slice(zero_den.table().layer(0).second.words(), 2, 3, w) == Words(w, 0));
        EXPECT(zero_den.holds());
        size_t off[4] = {mult[0], mult[1], mult[2] + 1, mult[3]};
        EXPECT(!build(beta_w, off).holds());
        const RqNTTVec z(cfg, uniform(f, 0x604, 1, w)), lam(cfg, uniform(f, 0x605, 1, w));
        auto claim = build(beta_w, mult).layer_claim(1, 1, z, lam);
        EXPECT(claim->sumcheck().message().len() >= 2);
    }
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
    for (const Family &f : fams) family_suite(f);
    std::printf(failures ? "lincomb api: %d FAILURES\n" : "lincomb api: all ok\n", failures);
    return failures ? 1 : 0;
}
