// IndexColumn, lincomb_index, lincomb_index_plan, from_u64, index_count, DenseMultilinearExtension::linear_combination_indexed,
// identity_permutation[_mles], permutation_leaves_indexed and LookupCheck::from_indices of include/stark_rings.hpp against a
// term-at-a-time restatement whose products come from the oracle (libsr_oracle), whose sums are limb arithmetic modulo the base prime
// on the memory image and whose R::from(x) is x one() by doubling and adding: one ring per family, both kernels, masked rows,
// truncated columns, progressions up to 2^64 - 1, bit for bit; one permutation check and one lookup check from integers.
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

// x one() by doubling and adding, most significant bit first
static Words embed(const Family &f, uint64_t x, const Words &one) {
    const size_t limbs = f.prime.size(), w = one.size();
    Words acc(w, 0);
    for (int bit = 63; bit >= 0; bit--) {
        const Words twice(acc);
        for (size_t c = 0; c < w; c += limbs) add_mod(acc.data() + c, twice.data() + c, f.prime);
        if ((x >> bit) & 1)
            for (size_t c = 0; c < w; c += limbs) add_mod(acc.data() + c, one.data() + c, f.prime);
    }
    return acc;
}
static uint64_t value_of(const IndexColumn &c, size_t e) { return c.is_progression ? c.start + e : (e < c.values.size() ? c.values[e] : 0); }

// one term at a time: out_m[e] = [bit K+J] c_m[K+J] + sum_k [bit k] c_m[k] * T_k[e] + sum_j [bit K+j] c_m[K+j] * R::from(col_j[e])
static std::vector<Words> restate(const Family &f, const std::vector<Words> &tables, const std::vector<IndexColumn> &cols, const Words &coef,
                                  const std::vector<uint32_t> &uses, size_t n, size_t w, const Words &one) {
    const size_t limbs = f.prime.size(), K = tables.size(), T = K + cols.size();
    std::vector<Words> outs;
    for (size_t m = 0; m < uses.size(); m++) {
        Words out(n * w, 0), t(w);
        for (size_t e = 0; e < n; e++) {
            for (size_t k = 0; k < T; k++) {
                if (!((uses[m] >> k) & 1)) continue;
                if (k < K) {
                    if ((e + 1) * w > tables[k].size()) continue;
                    std::copy(tables[k].begin() + e * w, tables[k].begin() + (e + 1) * w, t.begin());
                } else {
                    t = embed(f, value_of(cols[k - K], e), one);
                }
                f.mul(t.data(), coef.data() + (m * (T + 1) + k) * w);
                for (size_t c = 0; c < w; c += limbs) add_mod(out.data() + e * w + c, t.data() + c, f.prime);
            }
            if ((uses[m] >> T) & 1)
                for (size_t c = 0; c < w; c += limbs) add_mod(out.data() + e * w + c, coef.data() + (m * (T + 1) + T) * w + c, f.prime);
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

// stored values: the edges of a u64 and of the base prime where it is below 2^64
static Words edges(const Family &f, size_t count, size_t shift) {
    Words pool = {0, 1, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x8000000000000000ull, ~0ull};
    if (f.prime.size() == 1)
        for (uint64_t d : {(uint64_t)0, (uint64_t)1, (uint64_t)2}) pool.push_back(f.prime[0] - 1 + d);
    Words out;
    for (size_t i = 0; i < count; i++) out.push_back(pool[(i + shift) % pool.size()]);
    return out;
}

static void family_suite(const Family &f) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const int limbs = sro_limbs(f.field);
    const size_t w = cfg.words_per_elem(), n = 9;
    Words one(w, 0), m1(limbs), std1(limbs, 0);
    std1[0] = 1;
    sro_to_mont(f.field, std1.data(), m1.data(), 1);
    for (size_t i = 0; i < f.degree; i += f.slot_w) std::copy(m1.begin(), m1.end(), one.begin() + i * limbs);
    const RqNTTVec one_v(cfg, one);
    // both kernels (K + J = 3 / 5 / 16), several launches (M = 4), no table at all, masks, truncation, progressions up to 2^64 - 1
    const size_t shapes[][3] = {{0, 1, 1}, {1, 2, 2}, {3, 2, 1}, {0, 8, 2}, {8, 8, 4}};
    for (const auto &sh : shapes) {
        const size_t K = sh[0], J = sh[1], M = sh[2], T = K + J;
        std::vector<Words> tables;
        for (size_t k = 0; k < K; k++) tables.push_back(uniform(f, 0x100 * T + k, k % 3 == 1 ? n - 1 : n, w));
        std::vector<IndexColumn> cols;
        for (size_t j = 0; j < J; j++) {
            if (j % 3 == 1) cols.push_back(IndexColumn::progression(j % 2 ? ~0ull - (n - 1) : 0));
            else cols.push_back(IndexColumn::stored(edges(f, j == 2 ? n - 1 : (j == 5 ? 0 : n), j)));
        }
        const Words coef = uniform(f, 0x7000 + 16 * T + M, M * (T + 1), w);
        std::vector<uint32_t> uses(M, ((uint32_t)2 << T) - 1);
        if (M > 1 && T > 1) uses[1] = (((uint32_t)1 << T) - 1) & ~2u;   // no term 1, no constant
        std::vector<const Words *> ptrs;
        for (const Words &t : tables) ptrs.push_back(&t);
        const auto got = lincomb_index(cfg, ptrs, cols, coef, uses, n);
        const auto want = restate(f, tables, cols, coef, uses, n, w, one);
        EXPECT(got == want);
        if (got != want) std::printf("  %s K %zu J %zu M %zu\n", f.name, K, J, M);
        const auto plan = lincomb_index_plan(f.ring, f.log2d, (int)K, (int)J, (int)M);
        EXPECT(plan.first * plan.second >= (int)M && plan.second >= 1 && plan.second <= (int)M);
    }
    {   // no index column: sr_lincomb's words
        const Words t0 = uniform(f, 0x200, n, w), t1 = uniform(f, 0x201, n - 2, w), coef = uniform(f, 0x202, 3, w);
        EXPECT(lincomb_index(cfg, {&t0, &t1}, {}, coef, {0x7u}, n) == lincomb(cfg, {&t0, &t1}, coef, {0x7u}, n));
    }
    {   // from_u64 and the reference's fixtures: chunk i starts at i 2^num_vars
        const Words vals = edges(f, 11, 0);
        const Words got = from_u64(cfg, IndexColumn::stored(vals), vals.size(), one);
        for (size_t i = 0; i < vals.size(); i++) EXPECT(slice(got, i, i + 1, w) == embed(f, vals[i], one));
        const Words whole = identity_permutation(cfg, 2, 3, one_v);
        const auto mles = identity_permutation_mles(cfg, 2, 3, one_v);
        EXPECT(whole.size() == 12 * w && mles.size() == 3);
        for (size_t i = 0; i < mles.size(); i++) {
            EXPECT(mles[i].num_vars() == 2 && mles[i].words() == slice(whole, 4 * i, 4 * i + 4, w));
            EXPECT(slice(mles[i].words(), 0, 1, w) == embed(f, 4 * i, one));
        }
        EXPECT(slice(whole, 11, 12, w) == embed(f, 11, one));
    }
    {   // the class: two truncated MLEs in three variables beside a stored column and a progression, with and without the constant
        std::vector<DenseMultilinearExtension> mles;
        std::vector<Words> tables;
        for (size_t k = 0; k < 2; k++) {
            tables.push_back(uniform(f, 0x300 + k, k == 1 ? 0 : 5, w));
            mles.emplace_back(cfg, 3, tables.back());
        }
        const std::vector<IndexColumn> cols = {IndexColumn::stored(edges(f, 6, 3)), IndexColumn::progression(40)};
        const Words cw = uniform(f, 0x310, 5, w);
        const RqNTTVec coeffs(cfg, slice(cw, 0, 4, w)), constant(cfg, slice(cw, 4, 5, w));
        const auto a = DenseMultilinearExtension::linear_combination_indexed(cfg, 3, {&mles[0], &mles[1]}, cols, coeffs);
        EXPECT(a.num_vars() == 3 && a.len() == 8 && a.words() == restate(f, tables, cols, cw, {0xFu}, 8, w, one)[0]);
        const auto b = DenseMultilinearExtension::linear_combination_indexed(cfg, 3, {&mles[0], &mles[1]}, cols, coeffs, &constant);
        EXPECT(b.len() == 8 && b.words() == restate(f, tables, cols, cw, {0x1Fu}, 8, w, one)[0]);
        const auto c = DenseMultilinearExtension::linear_combination_indexed(cfg, 3, {&mles[0]}, {cols[0]}, RqNTTVec(cfg, slice(cw, 0, 2, w)));
        EXPECT(c.len() == 6);
        EXPECT_THROWS(DenseMultilinearExtension::linear_combination_indexed(cfg, 3, {&mles[0]}, cols, coeffs));
        EXPECT_THROWS(DenseMultilinearExtension::linear_combination_indexed(cfg, 2, {}, {IndexColumn::stored(edges(f, 5, 0))}, RqNTTVec(cfg, slice(cw, 0, 1, w))));
    }
    {   // refusals of the host form
        const Words t = uniform(f, 0x400, n, w), coef = uniform(f, 0x401, 3, w);
        const IndexColumn col = IndexColumn::stored(edges(f, n, 0));
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {col}, coef, {0x0u}, n));        // an empty mask
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {col}, coef, {0x8u}, n));        // a bit above K + J
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {col}, coef, {0x5u}, n));        // the column unused
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {col}, coef, {0x6u}, n));        // the table unused
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {col}, coef, {0x7u}, n - 1));    // n_evals > n
        EXPECT_THROWS(lincomb_index(cfg, {&t}, {IndexColumn::progression(~0ull - (n - 2))}, coef, {0x7u}, n));   // wraps
        EXPECT_THROWS(lincomb_index(cfg, {}, {}, coef, {0x1u}, n));
        EXPECT_THROWS(lincomb_index_plan(f.ring, f.log2d, 9, 8, 1));
        EXPECT_THROWS(lincomb_index_plan(f.ring, f.log2d, 1, 9, 1));
        EXPECT(lincomb_index(cfg, {&t}, {IndexColumn::progression(~0ull - (n - 1))}, coef, {0x7u}, n).size() == 1);   // the last that does not wrap
        EXPECT(index_count(cfg, {3, 0, 3, 3, 1}, 5) == Words({1, 1, 0, 3, 0}));
        EXPECT(index_count(cfg, {}, 3) == Words({0, 0, 0}));
        EXPECT_THROWS(index_count(cfg, {3, 5}, 5));
    }
    {   // a permutation check from a u64 sigma: 2^4 rows, f constant on the cycles of sigma
        const size_t rows = 16;
        const std::vector<std::vector<size_t>> cycles = {{0, 3, 7}, {1, 2}, {4, 9, 12, 15}, {6, 14, 8}};
        Words sigma(rows), fw;
        std::vector<size_t> cls(rows);
        for (size_t i = 0; i < rows; i++) {
            sigma[i] = i;
            cls[i] = cycles.size() + i;
        }
        for (size_t c = 0; c < cycles.size(); c++)
            for (size_t i = 0; i < cycles[c].size(); i++) {
                sigma[cycles[c][i]] = cycles[c][(i + 1) % cycles[c].size()];
                cls[cycles[c][i]] = c;
            }
        const Words values = uniform(f, 0x500, rows + cycles.size(), w);
        for (size_t i = 0; i < rows; i++) fw.insert(fw.end(), values.begin() + cls[i] * w, values.begin() + (cls[i] + 1) * w);
        const RqNTTVec beta(cfg, uniform(f, 0x502, 1, w)), gamma(cfg, uniform(f, 0x503, 1, w));
        auto build = [&](const Words &fv) {
            const auto nd = permutation_leaves_indexed(cfg, fv, sigma, beta, gamma, one_v);
            return PermutationCheck(cfg, nd.first, nd.second, 4);
        };
        const PermutationCheck ok = build(fw);
        EXPECT(ok.holds());
        // against permutation_leaves over tables made by from_u64
        const Words ident = from_u64(cfg, IndexColumn::progression(0), rows, one), sig = from_u64(cfg, IndexColumn::stored(sigma), rows, one);
        const auto nd = permutation_leaves(cfg, fw, ident, sig, beta, gamma, one_v);
        EXPECT(ok.num().layer(0).words() == nd.first && ok.den().layer(0).words() == nd.second);
        Words bad(fw);
        std::swap_ranges(bad.begin() + 3 * w, bad.begin() + 4 * w, bad.begin() + 9 * w);   // rows of two different cycles
        EXPECT(!build(bad).holds());
    }
    {   // a lookup from indices: 2^3 witness rows from a 2^2-row table of a ring column and an integer column
        const Words c0 = uniform(f, 0x600, 4, w), gm = uniform(f, 0x602, 1, w), ints = {7, 1ull << 40, 0, 12};
        const Words picks = {0, 2, 2, 3, 0, 2, 3, 1};
        Words w0, wi;
        for (uint64_t i : picks) {
            w0.insert(w0.end(), c0.begin() + i * w, c0.begin() + (i + 1) * w);
            wi.push_back(ints[i]);
        }
        Words minus_one(one), minus_gamma(gm);
        for (size_t c = 0; c < w; c += limbs) {
            neg_mod(minus_one.data() + c, f.prime);
            neg_mod(minus_gamma.data() + c, f.prime);
        }
        Words cw(minus_one);
        cw.insert(cw.end(), minus_gamma.begin(), minus_gamma.end());
        const Words beta_w = uniform(f, 0x603, 1, w);
        cw.insert(cw.end(), beta_w.begin(), beta_w.end());
        auto q = [&](const Words &col, const Words &iv) { return std::move(lincomb_index(cfg, {&col}, {IndexColumn::stored(iv)}, cw, {0x7u}, iv.size())[0]); };
        const LookupCheck ok = LookupCheck::from_indices(cfg, q(w0, wi), q(c0, ints), picks, 3, 2, one_v);
        EXPECT(ok.holds());
        const Words mult = from_u64(cfg, IndexColumn::stored({2, 1, 3, 2}), 4, one);
        EXPECT(ok.table().layer(0).first.words() == mult);
        Words off(wi);
        off[5] = 999;
        EXPECT(!LookupCheck::from_indices(cfg, q(w0, off), q(c0, ints), picks, 3, 2, one_v).holds());
        EXPECT_THROWS(LookupCheck::from_indices(cfg, q(w0, wi), q(c0, ints), {0, 4}, 3, 2, one_v));
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
    std::printf(failures ? "index api: %d FAILURES\n" : "index api: all ok\n", failures);
    return failures ? 1 : 0;
}
