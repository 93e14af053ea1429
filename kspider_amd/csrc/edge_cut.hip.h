// The containment columns of one join record, as the pairwise writer computes them, and the cut over them: shared by the
// clustering (cluster.hip) and the neighbour counts (repr.hip), which both read ksp_edge records in device memory.
#ifndef KSPIDER_EDGE_CUT_HIP_H
#define KSPIDER_EDGE_CUT_HIP_H
#include <cstdint>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"

// Column col (3 min, 4 avg, 5 max containment) of edge x: single-precision maths of the pairwise writer,
// index_io.cpp::format_rows = src/pairwise.cpp:260-264.  cnt[v] = k-mer count of source v.
__device__ inline float edge_col_value(const ksp_edge& x, const uint32_t* __restrict__ cnt, const int col) {
    const float n1 = (float)cnt[x.source_1], n2 = (float)cnt[x.source_2];
    const float c12 = (float)x.shared / n2, c21 = (float)x.shared / n1;
    float v;
    if (col == 3) v = c21 < c12 ? c21 : c12;        // std::min(c12, c21)
    else if (col == 5) v = c12 < c21 ? c21 : c12;   // std::max(c12, c21)
    else v = (float)((double)(c12 + c21) / 2.0);
    return v;
}

// Columns 3, 4 and 5 of edge x at once, from one pair of divisions: the same operations in the same order as edge_col_value
// (and as the writer), so each value is bit for bit the one edge_col_value returns for its column.
__device__ inline void edge_col_values(const ksp_edge& x, const uint32_t* __restrict__ cnt, float* mn, float* av, float* mx) {
    const float n1 = (float)cnt[x.source_1], n2 = (float)cnt[x.source_2];
    const float c12 = (float)x.shared / n2, c21 = (float)x.shared / n1;
    *mn = c21 < c12 ? c21 : c12;                   // std::min(c12, c21)
    *av = (float)((double)(c12 + c21) / 2.0);
    *mx = c12 < c21 ? c21 : c12;                   // std::max(c12, c21)
}

// An edge counts for the clustering when its containment column is not below the cut.  `vcrit` is the smallest float the
// reference's test (text of the float with 6 significant digits -> Python float -> x 100 -> not below cutoff x 100,
// ks_clustering.py:101-105) lets through: that test is monotone in the float, so one compare against the critical value
// found on the host (ksp::cc_critical) IS that test, digit for digit.
// mode 1: no finite value passes, only NaN rows do (a NaN is never "below": kept, as in the reference).
__device__ inline bool cc_edge_kept(const ksp_edge& x, const uint32_t* __restrict__ cnt, const int col, const float vcrit, const int mode) {
    const float v = edge_col_value(x, cnt, col);
    if (mode) return v != v;
    return !(v < vcrit);
}
#endif
