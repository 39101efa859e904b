// RqPolyVec::linf_norm / l2_norm_squared (+ _per_element) of include/stark_rings.hpp and CyclotomicConfig::norm_plan against the
// definition (crates/ring/src/traits.rs:6-36, balanced_decomposition/convertible_ring.rs:49-66): the standard-form value comes from
// the oracle (sro_from_mont), the signed representative, the maximum and the sum of squares are computed here -- with unsigned
// __int128 and a carry word for the one-limb rings, with schoolbook limbs for Stark.  Every output word is compared.
#include <cstdio>
#include <cstdlib>
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

// |signed representative| of one standard-form coefficient of `limbs` words (p given the same way): x if 2x < p, else p - x
static void magnitude(uint64_t *m, const uint64_t *x, const uint64_t *p, int limbs) {
    // x > (p - 1) / 2  <=>  2x >= p (p odd): compare 2x with p from the top
    uint64_t dbl[5] = {0, 0, 0, 0, 0}, pp[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < limbs; i++) {
        dbl[i] |= x[i] << 1;
        dbl[i + 1] = x[i] >> 63;
        pp[i] = p[i];
    }
    bool ge = true;
    for (int i = limbs; i >= 0; i--)
        if (dbl[i] != pp[i]) {
            ge = dbl[i] > pp[i];
            break;
        }
    uint64_t borrow = 0;
    for (int i = 0; i < limbs; i++) {
        const u128 d = (u128)p[i] - x[i] - borrow;
        m[i] = ge ? (uint64_t)d : x[i];
        borrow = (uint64_t)(d >> 64) & 1;
    }
}
// acc (n words) += a^2, a of `limbs` words: schoolbook on 64-bit words, every partial product added at its place with full carry
static void add_square(uint64_t *acc, int n, const uint64_t *a, int limbs) {
    for (int i = 0; i < limbs; i++)
        for (int j = 0; j < limbs; j++) {
            const u128 pr = (u128)a[i] * a[j];
            u128 c = (u128)acc[i + j] + (uint64_t)pr;
            acc[i + j] = (uint64_t)c;
            c = (c >> 64) + (uint64_t)(pr >> 64);
            for (int k = i + j + 1; k < n && c; k++) {
                c += acc[k];
                acc[k] = (uint64_t)c;
                c >>= 64;
            }
        }
}
static bool greater(const uint64_t *a, const uint64_t *b, int limbs) {
    for (int i = limbs - 1; i >= 0; i--)
        if (a[i] != b[i]) return a[i] > b[i];
    return false;
}

struct Family {
    const char *name;
    sr_ring ring;
    int field, log2d;
    uint64_t p[4];
};

static void expected(const Family &f, const Words &mont, size_t group, Words &linf, Words &l2) {
    const int limbs = sro_limbs(f.field), sw = limbs == 1 ? 3 : 9;
    const size_t n = mont.size() / limbs;
    Words std_form(mont.size());
    sro_from_mont(f.field, mont.data(), std_form.data(), n);
    linf.assign(n / group * limbs, 0);
    l2.assign(n / group * sw, 0);
    for (size_t i = 0; i < n; i++) {
        uint64_t m[4];
        magnitude(m, &std_form[i * limbs], f.p, limbs);
        uint64_t *mx = &linf[i / group * limbs];
        if (greater(m, mx, limbs))
            for (int k = 0; k < limbs; k++) mx[k] = m[k];
        if (limbs == 1) {  // the one-limb rings: one 128-bit square and a carry word
            uint64_t *s = &l2[i / group * 3];
            const u128 sq = (u128)m[0] * m[0], lo = ((u128)s[1] << 64 | s[0]) + sq;
            if (lo < sq) s[2]++;
            s[0] = (uint64_t)lo;
            s[1] = (uint64_t)(lo >> 64);
        } else {
            add_square(&l2[i / group * sw], sw, m, limbs);
        }
    }
}

static void run(const Family &f, size_t batch) {
    CyclotomicConfig cfg(f.ring, f.log2d);
    const int limbs = cfg.limbs();
    const size_t d = cfg.dimension(), n = batch * d;
    Words w(n * limbs);
    sro_fill_uniform(f.field, 0x4E02 + f.ring, 0, n, w.data());
    // the extremes of the signed representative at both ends: p - 1 -> 1, (p - 1) / 2 and (p + 1) / 2 -> (p - 1) / 2
    Words edge(3 * limbs, 0), edge_m(3 * limbs);
    for (int k = 0; k < limbs; k++) edge[k] = f.p[k], edge[limbs + k] = f.p[k], edge[2 * limbs + k] = f.p[k];
    edge[0] -= 1;                                        // p - 1 (p is odd and its low word is not zero)
    for (int k = 0; k < limbs; k++) {                    // (p - 1) / 2, then (p + 1) / 2 = that + 1
        const uint64_t hi = k + 1 < limbs ? f.p[k + 1] : 0, lo = k == 0 ? f.p[0] - 1 : f.p[k];
        edge[limbs + k] = (lo >> 1) | (hi << 63);
        edge[2 * limbs + k] = edge[limbs + k];
    }
    edge[2 * limbs] += 1;  // no carry: the low word of (p - 1) / 2 is even or far from 2^64 - 1 for these primes
    sro_to_mont(f.field, edge.data(), edge_m.data(), 3);
    for (int k = 0; k < limbs; k++) {
        w[k] = edge_m[k];
        w[(n / 2) * limbs + k] = edge_m[limbs + k];
        w[(n - 1) * limbs + k] = edge_m[2 * limbs + k];
    }
    RqPolyVec v(cfg, w);
    Words linf, l2;
    expected(f, w, n, linf, l2);
    EXPECT(v.linf_norm() == linf);
    EXPECT(v.l2_norm_squared() == l2);
    expected(f, w, d, linf, l2);
    EXPECT(v.linf_norm_per_element() == linf);
    EXPECT(v.l2_norm_squared_per_element() == l2);
    const CyclotomicConfig::NormPlan p = cfg.norm_plan(n, n, SR_NORM_LINF | SR_NORM_L2SQ);
    EXPECT(p.words_per_group == (size_t)(limbs == 1 ? 4 : 13) && p.launches >= 1 && p.launches <= 2);
    // an empty vector: l2 = 0, linf throws
    RqPolyVec none(cfg, Words());
    EXPECT(none.l2_norm_squared() == Words(limbs == 1 ? 3 : 9, 0));
    bool threw = false;
    try {
        none.linf_norm();
    } catch (const std::runtime_error &) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s ok so far (failures %d)\n", f.name, failures);
}

int main() {
    const uint64_t gl = 0xFFFFFFFF00000001ull, bb = 2013265921ull, frog = 0xDCD31BD79EC2DD19ull;
    const Family fams[] = {
        {"goldilocks 2^10", SR_RING_GOLDILOCKS_POW2, 0, 10, {gl, 0, 0, 0}},
        {"babybear 2^12", SR_RING_BABYBEAR_POW2, 1, 12, {bb, 0, 0, 0}},
        {"stark 2^6", SR_RING_STARK_POW2, 2, 6, {1, 0, 0, 0x0800000000000011ull}},
        {"goldilocks24", SR_RING_GOLDILOCKS_24, 0, 0, {gl, 0, 0, 0}},
        {"babybear72", SR_RING_BABYBEAR_72, 1, 0, {bb, 0, 0, 0}},
        {"frog16", SR_RING_FROG_16, 3, 0, {frog, 0, 0, 0}},
    };
    for (const Family &f : fams) run(f, 37);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
