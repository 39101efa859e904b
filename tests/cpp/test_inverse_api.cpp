// RqNTTVec::inverse / divide / inverse_zero_count and DenseMultilinearExtension::inverse / divide of include/stark_rings.hpp against
// vectors written by tests/test_cpp_inverse_api.py (Python integers for the power-of-two rings, the vectors' own defining property
// y * den == num through operator* for the reference's own rings), bit for bit.
// File of little-endian u64 words: the number of cases, then per case ring, log2 D, words per element, n, the zero slots planted, a
// flag (1: the expected words follow) and den, num [, 1 / den, num / den] of n elements each.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../include/stark_rings.hpp"

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

static Words take(const Words &all, size_t &pos, size_t n) {
    if (pos + n > all.size()) {
        std::printf("vector file too short\n");
        std::exit(2);
    }
    Words out(all.begin() + pos, all.begin() + pos + n);
    pos += n;
    return out;
}
template <class E, class Fn>
static bool throws(Fn fn) {
    try {
        fn();
    } catch (const E &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    Words all;
    uint64_t word;
    while (std::fread(&word, 8, 1, f) == 1) all.push_back(word);
    std::fclose(f);
    size_t pos = 0;
    const size_t cases = take(all, pos, 1)[0];
    for (size_t c = 0; c < cases; c++) {
        const Words h = take(all, pos, 6);
        const size_t w = h[2], n = h[3], zeros = h[4];
        CyclotomicConfig cfg((sr_ring)h[0], (int)h[1]);
        EXPECT(cfg.words_per_elem() == w);
        const RqNTTVec den(cfg, take(all, pos, n * w)), num(cfg, take(all, pos, n * w));
        (void)den.inverse_zero_count();
        const RqNTTVec inv = den.inverse();
        EXPECT(den.inverse_zero_count() == zeros);
        EXPECT(den.inverse_zero_count() == 0);  // the read cleared it
        const RqNTTVec quo = num.divide(den);
        EXPECT(num.inverse_zero_count() == zeros);
        EXPECT(inv.len() == n && quo.len() == n);
        if (h[5]) {
            EXPECT(inv.words() == take(all, pos, n * w));
            EXPECT(quo.words() == take(all, pos, n * w));
        }
        // the defining property where no slot was zero: (num / den) * den == num, and num * (1 / den) == num / den everywhere
        if (zeros == 0) EXPECT(quo * den == num);
        EXPECT(num * inv == quo);
        // the MLE mirrors go over the same call
        const DenseMultilinearExtension md(cfg, 6, den.words()), mn(cfg, 6, num.words());
        EXPECT(md.inverse().words() == inv.words() && md.inverse().num_vars() == 6);
        EXPECT(mn.divide(md).words() == quo.words());
        EXPECT(md.inverse_zero_count() == 3 * zeros);
        // the empty vector: nothing to do, nothing counted
        const RqNTTVec none(cfg, Words());
        EXPECT(none.inverse().len() == 0 && none.divide(none).len() == 0 && none.inverse_zero_count() == 0);
        EXPECT(throws<std::length_error>([&] { num.divide(none); }));
        EXPECT(throws<std::length_error>([&] { mn.divide(DenseMultilinearExtension(cfg, 5, den.words())); }));
        std::printf("ring %d log2 D %d: done\n", (int)h[0], (int)h[1]);
    }
    EXPECT(pos == all.size());
    std::printf(failures ? "inverse api: %d FAILURES\n" : "inverse api: all ok\n", failures);
    return failures ? 1 : 0;
}
