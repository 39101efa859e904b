// DenseMultilinearExtension of include/stark_rings.hpp against a one-variable-at-a-time restatement of crates/poly
// (mle/dense.rs:171-199, polynomials/multilinear_polynomial.rs:251-286) whose products come from the oracle (libsr_oracle) and whose
// sums and differences are plain integer arithmetic modulo p: one fold per ring family, both orders, bit for bit.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../include/stark_rings.hpp"
#include "../../oracle/sr_oracle.h"

using namespace stark_rings;
typedef unsigned __int128 u128;
typedef std::vector<uint64_t> Words;

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

// a +- b modulo p on `limbs` little-endian words per coefficient (p given the same way)
static void addsub(uint64_t *out, const uint64_t *a, const uint64_t *b, const uint64_t *p, int limbs, bool sub) {
    uint64_t t[4], u[4];
    u128 c = 0;
    if (!sub) {
        for (int i = 0; i < limbs; i++) { c += (u128)a[i] + b[i]; t[i] = (uint64_t)c; c >>= 64; }
        // t (with carry c) >= p ? subtract p
        uint64_t borrow = 0;
        for (int i = 0; i < limbs; i++) { u128 d = (u128)t[i] - p[i] - borrow; u[i] = (uint64_t)d; borrow = (uint64_t)(d >> 64) & 1; }
        const bool ge = c || !borrow;
        for (int i = 0; i < limbs; i++) out[i] = ge ? u[i] : t[i];
    } else {
        uint64_t borrow = 0;
        for (int i = 0; i < limbs; i++) { u128 d = (u128)a[i] - b[i] - borrow; t[i] = (uint64_t)d; borrow = (uint64_t)(d >> 64) & 1; }
        c = 0;
        for (int i = 0; i < limbs; i++) { c += (u128)t[i] + p[i]; u[i] = (uint64_t)c; c >>= 64; }
        for (int i = 0; i < limbs; i++) out[i] = borrow ? u[i] : t[i];
    }
}

struct Family {
    const char *name;
    sr_ring ring;
    int field, log2d;
    size_t degree;
    uint64_t p[4];
    std::function<void(uint64_t *, const uint64_t *)> mul;  // lhs <- lhs * rhs, one ring element, slot-wise
};

// table: 2^nv elements of w words; returns the folded table
static Words restate(const Family &f, Words t, size_t nv, const Words &point, int order) {
    const int limbs = sro_limbs(f.field);
    const size_t w = f.degree * limbs, nf = point.size() / w;
    Words d(w);
    for (size_t step = 0; step < nf; step++) {
        const size_t half = (size_t)1 << (nv - 1);
        const uint64_t *r = point.data() + (order == SR_MLE_LEADING ? step : nf - 1 - step) * w;
        Words next(half * w);
        for (size_t b = 0; b < half; b++) {
            const uint64_t *lo = t.data() + (order == SR_MLE_LEADING ? 2 * b : b) * w;
            const uint64_t *hi = t.data() + (order == SR_MLE_LEADING ? 2 * b + 1 : b + half) * w;
            for (size_t i = 0; i < f.degree; i++) addsub(&d[i * limbs], hi + i * limbs, lo + i * limbs, f.p, limbs, true);
            f.mul(d.data(), r);
            for (size_t i = 0; i < f.degree; i++) addsub(&next[(b * f.degree + i) * limbs], lo + i * limbs, &d[i * limbs], f.p, limbs, false);
        }
        t.swap(next);
        nv--;
    }
    return t;
}

static void family_suite(const Family &f, size_t nv) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const size_t w = cfg.words_per_elem(), n_evals = ((size_t)1 << nv) - 3;
    Words table = uniform(f.field, 0xC0 + nv, n_evals * f.degree), point = uniform(f.field, 0xC1 + nv, nv * f.degree);
    Words padded(table);
    padded.resize(w << nv, 0);
    DenseMultilinearExtension mle(cfg, nv, table);
    EXPECT(mle.num_vars() == nv && mle.len() == n_evals);
    EXPECT(mle.to_evaluations().words() == padded);
    for (int order : {SR_MLE_LEADING, SR_MLE_TRAILING})
        for (size_t nf : {(size_t)0, (size_t)1, (size_t)3, nv}) {
            Words pt = order == SR_MLE_LEADING ? Words(point.begin(), point.begin() + nf * w) : Words(point.end() - nf * w, point.end());
            const Words want = restate(f, padded, nv, pt, order);
            RqNTTVec p(cfg, pt);
            const DenseMultilinearExtension got = order == SR_MLE_LEADING ? mle.fixed_variables(p) : mle.fix_last_variables(p);
            EXPECT(got.num_vars() == nv - nf);
            EXPECT(got.words() == want);
            if (got.words() != want) std::printf("  %s order %d n_fixed %zu\n", f.name, order, nf);
        }
    RqNTTVec whole(cfg, point);
    const Words value = restate(f, padded, nv, point, SR_MLE_LEADING);
    auto ev = mle.evaluate(whole);
    EXPECT(ev.has_value() && ev->words() == value);
    EXPECT(!mle.evaluate(RqNTTVec(cfg, Words(point.begin(), point.begin() + w))).has_value());
    DenseMultilinearExtension step(mle);
    step.fix_variables(RqNTTVec(cfg, Words(point.begin(), point.begin() + 2 * w)));
    step.fix_variables(RqNTTVec(cfg, Words(point.begin() + 2 * w, point.end())));
    EXPECT(step.num_vars() == 0 && step.words() == value);
    const auto plan = mle.plan(nv, SR_MLE_LEADING, f.log2d);
    EXPECT(plan.second >= 2 && plan.first > 0 && 4 * plan.first <= 3 * ((size_t)1 << nv));
    // acc += r * x against the same pieces
    Words x = uniform(f.field, 0xC2, n_evals * f.degree), r = uniform(f.field, 0xC3, f.degree), want(table);
    const int limbs = sro_limbs(f.field);
    for (size_t e = 0; e < n_evals; e++) {
        Words prod(x.begin() + e * w, x.begin() + (e + 1) * w);
        f.mul(prod.data(), r.data());
        for (size_t i = 0; i < f.degree; i++) addsub(&want[(e * f.degree + i) * limbs], &table[(e * f.degree + i) * limbs], &prod[i * limbs], f.p, limbs, false);
    }
    DenseMultilinearExtension acc(cfg, nv, table);
    acc.add_assign_scaled(RqNTTVec(cfg, r), DenseMultilinearExtension(cfg, nv, x));
    EXPECT(acc.words() == want);
    std::printf("%s: done\n", f.name);
}

int main() {
    const uint64_t GL = 0xFFFFFFFF00000001ull, BB = 2013265921ull, FROG = 15912092521325583641ull;
    auto pow2 = [](int field, size_t d) { return [field, d](uint64_t *l, const uint64_t *r) { sro_pow2_pointwise(field, l, r, d); }; };
    const Family fams[] = {
        {"goldilocks 2^6", SR_RING_GOLDILOCKS_POW2, 0, 6, 64, {GL, 0, 0, 0}, pow2(0, 64)},
        {"babybear 2^5", SR_RING_BABYBEAR_POW2, 1, 5, 32, {BB, 0, 0, 0}, pow2(1, 32)},
        {"stark 2^4", SR_RING_STARK_POW2, 2, 4, 16, {1, 0, 0, 0x0800000000000011ull}, pow2(2, 16)},
        {"goldilocks24", SR_RING_GOLDILOCKS_24, 0, 0, 24, {GL, 0, 0, 0}, sro_g24_ntt_mul},
        {"babybear72", SR_RING_BABYBEAR_72, 1, 0, 72, {BB, 0, 0, 0}, sro_bb72_ntt_mul},
        {"frog16", SR_RING_FROG_16, 3, 0, 16, {FROG, 0, 0, 0}, sro_frog16_ntt_mul},
    };
    for (const Family &f : fams) family_suite(f, 7);
    std::printf(failures ? "mle api: %d FAILURES\n" : "mle api: all ok\n", failures);
    return failures ? 1 : 0;
}
