// SymmetricMatrixNTT of include/stark_rings.hpp against vectors written by the Python restatement (tools/model_symmetric.py through
// tests/test_cpp_symm_api.py): the Gram matrix of a random matrix and its G^T M G recomposition, one case per ring family, bit for bit.
// File of little-endian u64 words: the number of cases, then per case ring, log2 D, n, d, m, words per element, and the words of
// a (n d x m elements), powers (d), gram(a) (packed, size n d) and its recomposition (packed, size n).
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
template <class Fn>
static bool throws_length_error(Fn fn) {
    try {
        fn();
    } catch (const std::length_error &) {
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
        const size_t n = h[2], d = h[3], m = h[4], w = h[5], nd = n * d;
        CyclotomicConfig cfg((sr_ring)h[0], (int)h[1]);
        EXPECT(cfg.words_per_elem() == w);
        const Words a = take(all, pos, nd * m * w), powers = take(all, pos, d * w);
        const Words want_gram = take(all, pos, nd * (nd + 1) / 2 * w), want_small = take(all, pos, n * (n + 1) / 2 * w);
        const SymmetricMatrixNTT g = SymmetricMatrixNTT::gram(RqNTTVec(cfg, a), nd, m);
        EXPECT(g.size() == nd && g.words() == want_gram);
        const RqNTTVec p(cfg, powers);
        const SymmetricMatrixNTT small = recompose_left_right_symmetric_matrix(g, p);
        EXPECT(small.size() == n && small.words() == want_small);
        EXPECT(g.recompose_left_right(p).words() == want_small);
        // the accessors on the packed layout
        Words diag;
        for (size_t i = 0; i < nd; i++)
            for (size_t j = 0; j < nd; j++) {
                const size_t e = j <= i ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i;
                const Words elem(want_gram.begin() + e * w, want_gram.begin() + (e + 1) * w);
                EXPECT(g.at(i, j).words() == elem);
                if (i == j) diag.insert(diag.end(), elem.begin(), elem.end());
            }
        EXPECT(g.diag().words() == diag);
        const std::vector<RqNTTVec> rows = g.rows();
        EXPECT(rows.size() == nd);
        for (size_t i = 0; i < rows.size(); i++) EXPECT(rows[i].len() == i + 1);
        EXPECT(SymmetricMatrixNTT::from_rows(cfg, rows).words() == want_gram);
        // where the reference asserts
        std::vector<RqNTTVec> bad(rows);
        bad.back() = rows.front();
        if (nd > 1) EXPECT(throws_length_error([&] { SymmetricMatrixNTT::from_rows(cfg, bad); }));
        EXPECT(throws_length_error([&] { g.recompose_left_right(RqNTTVec(cfg, Words())); }));                       // d == 0
        EXPECT(throws_length_error([&] { g.recompose_left_right(RqNTTVec(cfg, Words((nd + 1) * w, 0))); }));      // nd + 1 does not divide nd
        EXPECT(throws_length_error([&] { SymmetricMatrixNTT(cfg, nd, Words(w, 0)); }) == (nd != 1));
        const SymmetricMatrixNTT z = SymmetricMatrixNTT::zero(cfg, 3);
        EXPECT(z.size() == 3 && z.words() == Words(6 * w, 0));
        EXPECT(SymmetricMatrixNTT::gram(RqNTTVec(cfg, Words()), 3, 0).words() == z.words());                     // m == 0: all zero()
        EXPECT(SymmetricMatrixNTT::gram(RqNTTVec(cfg, Words()), 0, 4).size() == 0);
        const auto gp = SymmetricMatrixNTT::gram_plan((sr_ring)h[0], (int)h[1], nd, m);
        const auto rp = SymmetricMatrixNTT::recompose_plan((sr_ring)h[0], (int)h[1], n, d);
        EXPECT(gp.second >= 1 && (gp.first == 0) == (gp.second == 1));
        EXPECT(rp.first == d * d && rp.second == 2);
        std::printf("ring %d log2 D %d: done\n", (int)h[0], (int)h[1]);
    }
    EXPECT(pos == all.size());
    std::printf(failures ? "symm api: %d FAILURES\n" : "symm api: all ok\n", failures);
    return failures ? 1 : 0;
}
