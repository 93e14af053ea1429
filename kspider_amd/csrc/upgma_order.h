// The order of candidate pairs of the average-linkage tree (upgma.hip), one function for the device's offer
// kernel, the host finish, the final sort of the rows and ksp_upgma_before.
//
// A pair is (S, P, lo, hi): S the sum of q between its two clusters, P = |lo's cluster| * |hi's cluster|, lo < hi the two roots.
// Its similarity is the rational S / P.  Pair 1 comes BEFORE pair 2 when
//   1. S1 / P1 > S2 / P2, compared exactly as S1 * P2 > S2 * P1 in 128 bits: S < 2^64 (fewer than 2^32 - 1 records of q <= 2^32)
//      and P < 2^64 (two sizes below 2^32), so a cross product is below 2^128 and cannot wrap;
//   2. else lo1 < lo2;
//   3. else hi1 < hi2.
// Two different pairs of one round never compare equal: they differ in (lo, hi).
#ifndef KSPIDER_UPGMA_ORDER_H
#define KSPIDER_UPGMA_ORDER_H
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KSP_UPGMA_HD __host__ __device__
#else
#define KSP_UPGMA_HD
#endif

KSP_UPGMA_HD inline bool ksp_upgma_pair_before(const uint64_t s1, const uint64_t p1, const uint32_t lo1, const uint32_t hi1, const uint64_t s2, const uint64_t p2,
                                               const uint32_t lo2, const uint32_t hi2) {
    const unsigned __int128 x = (unsigned __int128)s1 * p2, y = (unsigned __int128)s2 * p1;
    if (x != y) return x > y;
    if (lo1 != lo2) return lo1 < lo2;
    return hi1 < hi2;
}
#endif
