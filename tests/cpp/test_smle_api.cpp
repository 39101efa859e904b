// SparseMultilinearExtension and eq_table of include/stark_rings.hpp against the reference's own vectors (crates/poly mle/sparse.rs:463-510,
// the numbers of tests/golden/sparse_mle_kats.json): integers embedded as constant ring elements, goldilocks D = 2^6 and goldilocks24.
#include <cstdio>
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

static const int kGoldilocks = 0;  // the oracle's field id

// n copies of the constant element `value` in CRT/NTT form: zero plus the scalar in every slot
static RqNTTVec constants(const CyclotomicConfig &cfg, const std::vector<uint64_t> &values) {
    Words w;
    for (uint64_t v : values) {
        uint64_t m;
        sro_to_mont(kGoldilocks, &v, &m, 1);
        RqNTTVec e(cfg, Words(cfg.words_per_elem(), 0));
        e += Words{m};
        w.insert(w.end(), e.words().begin(), e.words().end());
    }
    return RqNTTVec(cfg, std::move(w));
}
static RqNTTVec bits(const CyclotomicConfig &cfg, size_t index, size_t n) {
    std::vector<uint64_t> b(n);
    for (size_t i = 0; i < n; i++) b[i] = (index >> i) & 1;
    return constants(cfg, b);
}

static void run(const char *name, sr_ring ring, int log2d) {
    CyclotomicConfig cfg(ring, log2d);
    // test_vec_to_mle
    const std::vector<uint64_t> z = {3, 1, 35, 9, 27, 30};
    SparseMultilinearExtension zm = SparseMultilinearExtension::from_slice(3, constants(cfg, z));
    for (size_t i = 0; i < 8; i++) EXPECT(zm.evaluate(bits(cfg, i, 3)) == constants(cfg, {i < z.size() ? z[i] : 0}));
    // eq table: sum_b eq[b] = one(), and a boolean point selects one entry
    RqNTTVec eq = eq_table(bits(cfg, 5, 3));
    EXPECT(eq.len() == 8 && eq.sum() == constants(cfg, {1}));
    for (size_t b = 0; b < 8; b++) {
        Words e(eq.words().begin() + b * cfg.words_per_elem(), eq.words().begin() + (b + 1) * cfg.words_per_elem());
        EXPECT(RqNTTVec(cfg, e) == constants(cfg, {b == 5 ? 1u : 0u}));
    }
    EXPECT(eq_table(RqNTTVec(cfg, Words())) == constants(cfg, {1}));
    // test_matrix_to_mle
    const std::vector<std::vector<uint64_t>> m4 = {{2, 3, 4, 4}, {4, 11, 14, 14}, {2, 8, 17, 17}, {420, 4, 2, 0}};
    const std::vector<std::vector<uint64_t>> m5 = {{2, 3, 4, 4, 1}, {4, 11, 14, 14, 2}, {2, 8, 17, 17, 3}, {420, 4, 2, 0, 4}, {420, 4, 2, 0, 5}};
    const struct {
        const std::vector<std::vector<uint64_t>> *m;
        size_t entries, num_vars;
    } cases[] = {{&m4, 15, 4}, {&m5, 23, 6}};
    for (const auto &c : cases) {
        std::vector<uint64_t> vals, row_ptr = {0};
        std::vector<uint32_t> cols;
        for (const auto &row : *c.m) {
            for (size_t j = 0; j < row.size(); j++)
                if (row[j]) {
                    vals.push_back(row[j]);
                    cols.push_back((uint32_t)j);
                }
            row_ptr.push_back(cols.size());
        }
        const size_t n = c.m->size();
        SparseMultilinearExtension a = SparseMultilinearExtension::from_matrix(constants(cfg, vals), cols, row_ptr, n, n);
        EXPECT(a.len() == c.entries && a.num_vars() == c.num_vars);
        const size_t n_cols = n == 4 ? 4 : 8;
        for (size_t r = 0; r < n; r++)
            for (size_t col = 0; col < n_cols; col++)
                EXPECT(a.evaluate(bits(cfg, r * n_cols + col, c.num_vars)) == constants(cfg, {col < n ? (*c.m)[r][col] : 0}));
        // fixing the column variables leaves one entry per row; the dense table of the result has 2^(num_vars - s) elements
        SparseMultilinearExtension rows = a.fixed_variables(bits(cfg, 1, n == 4 ? 2 : 3));
        EXPECT(rows.len() == n && rows.to_evaluations().len() == ((size_t)1 << rows.num_vars()));
        for (size_t r = 0; r < n; r++) {
            Words e(rows.words().begin() + r * cfg.words_per_elem(), rows.words().begin() + (r + 1) * cfg.words_per_elem());
            EXPECT(rows.indices()[r] == r && RqNTTVec(cfg, e) == constants(cfg, {(*c.m)[r][1]}));
        }
    }
    bool threw = false;
    try {
        SparseMultilinearExtension(cfg, 2, {1, 1}, constants(cfg, {1, 2}).words());
    } catch (const std::exception &) {
        threw = true;
    }
    EXPECT(threw);
    std::printf("%s done\n", name);
}

int main() {
    run("goldilocks", SR_RING_GOLDILOCKS_POW2, 6);
    run("goldilocks24", SR_RING_GOLDILOCKS_24, 0);
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("all ok\n");
    return 0;
}
