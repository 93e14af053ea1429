// ORACLE — TEST INFRASTRUCTURE ONLY.
//
// scipy's pdist(M, 'euclidean') between the ROWS of a matrix, in square form, restated for the export's single
// linkage (the numpy restatement is tests/export_restate.py: row_pdist).  Per pair, a sequential sum
// over the columns in ascending order of (M[i][c] - M[j][c])^2, each operation rounded on its own, then sqrt.  A column
// where both rows are 0 adds (0 - 0)^2 = +0, which leaves a sum >= +0 as it is, so only the columns where either row is
// nonzero are visited: a merge of the two rows' sorted nonzero columns.  That makes a matrix with a few dozen nonzeros
// per row cost O(n^2 x nonzeros) instead of O(n^3).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "oracle.h"

namespace {

struct SparseRows {
    std::vector<uint64_t> off;
    std::vector<uint32_t> col;
    std::vector<double> val;
};

SparseRows sparse_rows(const double* M, uint64_t ld, uint32_t n) {
    SparseRows s;
    s.off.assign(1, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const double* row = M + (uint64_t)i * ld;
        for (uint32_t c = 0; c < n; ++c)
            if (row[c] != 0.0) {
                s.col.push_back(c);
                s.val.push_back(row[c]);
            }
        s.off.push_back(s.col.size());
    }
    return s;
}

double pair_sum(const SparseRows& s, uint32_t i, uint32_t j) {
    uint64_t a = s.off[i], b = s.off[j];
    const uint64_t ae = s.off[i + 1], be = s.off[j + 1];
    double sum = 0.0;   // (built with -ffp-contract=off: d * d and the addition stay two roundings)
    while (a < ae || b < be) {
        double d;
        if (b == be || (a < ae && s.col[a] < s.col[b])) {
            d = s.val[a++];
        } else if (a == ae || s.col[b] < s.col[a]) {
            d = 0.0 - s.val[b++];
        } else {
            d = s.val[a++] - s.val[b++];
        }
        const double t = d * d;
        sum = sum + t;
    }
    return sum;
}

}  // namespace

extern "C" int oracle_row_pdist(const double* M, uint64_t ld, uint32_t n, double* out, int threads) {
    if (!M || !out || ld < n) return 1;
    const SparseRows s = sparse_rows(M, ld, n);
    std::atomic<uint32_t> next{0};
    auto work = [&] {
        for (uint32_t i; (i = next.fetch_add(1)) < n;) {
            out[(uint64_t)i * n + i] = 0.0;
            for (uint32_t j = i + 1; j < n; ++j)   // ((a - b)^2 == (b - a)^2: the sum of (i, j) is that of (j, i))
                out[(uint64_t)i * n + j] = out[(uint64_t)j * n + i] = std::sqrt(pair_sum(s, i, j));
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < std::max(1, threads); ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    return 0;
}
