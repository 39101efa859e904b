// SparseMatrixNTT::transpose / checked_mul_mat / try_mul_mat and MatrixNTT::transpose of include/stark_rings.hpp against vectors written
// by the Python restatement (tools/model_sparse_matrix.py through tests/test_cpp_spgemm_api.py), one case per ring family, bit for bit.
// File of little-endian u64 words: the number of cases, then per case ring, log2 D, words per element, the number of products, per
// product the matrices A, B, A B and A^T, and last a matrix with unsorted rows and its transpose.  A matrix is nrows, ncols, nnz,
// row_ptr (nrows + 1), cols (nnz) and the words of the nnz stored elements.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "../../include/stark_rings.hpp"

using namespace stark_rings;
typedef std::vector<uint64_t> Words;
typedef std::vector<std::vector<SparseMatrixNTT::Entry>> Coeffs;

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
struct Mat {
    size_t nrows, ncols;
    Coeffs coeffs;
};
static Mat take_matrix(const Words &all, size_t &pos, size_t w) {
    const Words h = take(all, pos, 3);
    Mat m{(size_t)h[0], (size_t)h[1], Coeffs(h[0])};
    const Words row_ptr = take(all, pos, m.nrows + 1), cols = take(all, pos, h[2]), vals = take(all, pos, h[2] * w);
    for (size_t r = 0; r < m.nrows; r++)
        for (uint64_t t = row_ptr[r]; t < row_ptr[r + 1]; t++)
            m.coeffs[r].emplace_back(Words(vals.begin() + t * w, vals.begin() + (t + 1) * w), (size_t)cols[t]);
    return m;
}
static bool same(const SparseMatrixNTT &got, const Mat &want) {
    return got.nrows() == want.nrows && got.ncols() == want.ncols && got.coeffs() == want.coeffs;
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
        const Words h = take(all, pos, 4);
        const size_t w = h[2];
        CyclotomicConfig cfg((sr_ring)h[0], (int)h[1]);
        EXPECT(cfg.words_per_elem() == w);
        for (size_t q = 0; q < h[3]; q++) {
            const Mat a = take_matrix(all, pos, w), b = take_matrix(all, pos, w), ab = take_matrix(all, pos, w), at = take_matrix(all, pos, w);
            const SparseMatrixNTT sa(cfg, a.nrows, a.ncols, a.coeffs), sb(cfg, b.nrows, b.ncols, b.coeffs);
            EXPECT(sa.coeffs() == a.coeffs);
            const auto prod = sa.checked_mul_mat(sb);
            EXPECT(prod && same(*prod, ab));
            EXPECT(same(sa.try_mul_mat(sb), ab));
            const SparseMatrixNTT t = sa.transpose();
            EXPECT(same(t, at));
            EXPECT(same(t.transpose(), a));  // the rows of a ascend: transposing twice returns it
            // (A B)^T = B^T A^T holds entry by entry: the same products meet in the same entries, sums are exact
            EXPECT(same(sb.transpose().try_mul_mat(t), Mat{ab.ncols, ab.nrows, prod->transpose().coeffs()}));
            // where the reference returns None
            const SparseMatrixNTT wrong(cfg, b.nrows + 1, b.ncols, Coeffs(b.nrows + 1));
            EXPECT(!sa.checked_mul_mat(wrong));
            EXPECT(throws<std::length_error>([&] { sa.try_mul_mat(wrong); }));
            // an empty operand: no entry
            const SparseMatrixNTT none(cfg, b.nrows, b.ncols, Coeffs(b.nrows));
            EXPECT(same(sa.try_mul_mat(none), Mat{a.nrows, b.ncols, Coeffs(a.nrows)}));
        }
        const Mat u = take_matrix(all, pos, w), ut = take_matrix(all, pos, w);
        const SparseMatrixNTT su(cfg, u.nrows, u.ncols, u.coeffs);
        EXPECT(same(su.transpose(), ut));
        // rows that do not ascend strictly are refused by the product; a column past ncols by the transpose (the reference panics)
        const SparseMatrixNTT id(cfg, u.ncols, u.ncols, Coeffs(u.ncols));
        EXPECT(throws<std::runtime_error>([&] { su.checked_mul_mat(id); }));
        EXPECT(throws<std::runtime_error>([&] { SparseMatrixNTT(cfg, u.nrows, 1, u.coeffs).transpose(); }));
        EXPECT(same(SparseMatrixNTT(cfg, 0, 3, Coeffs()).transpose(), Mat{3, 0, Coeffs(3)}));
        // Matrix::transpose on the stored elements of u as a dense 2 x (nnz / 2) matrix: the data is transposed, the shape is that of the data
        const size_t half = su.nnz() / 2;
        Words dense, want(2 * half * w);
        for (const auto &row : u.coeffs)
            for (const auto &e : row)
                if (dense.size() < 2 * half * w) dense.insert(dense.end(), e.first.begin(), e.first.end());
        for (size_t i = 0; i < 2; i++)
            for (size_t j = 0; j < half; j++)
                for (size_t x = 0; x < w; x++) want[(j * 2 + i) * w + x] = dense[(i * half + j) * w + x];
        const MatrixNTT d(cfg, 2, half, dense), dt = d.transpose();
        EXPECT(half >= 2 && dt.nrows() == half && dt.ncols() == 2 && dt.words() == want);
        EXPECT(dt.transpose().words() == dense);
        EXPECT(MatrixNTT(cfg, 0, 4, Words()).transpose().nrows() == 4);
        std::printf("ring %d log2 D %d: done\n", (int)h[0], (int)h[1]);
    }
    EXPECT(pos == all.size());
    std::printf(failures ? "spgemm api: %d FAILURES\n" : "spgemm api: all ok\n", failures);
    return failures ? 1 : 0;
}
