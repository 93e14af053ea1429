// Average ANI of a pairwise row (`kSpider pairwise --estimate-ani`, pykSpider/kSpider2/ks_pairwise.py:29-84), one
// definition for the host and the device.
//
// The reference reads columns 3 (min containment) and 5 (max containment) of the pairwise TSV as Python floats and
// hands each to sourmash.distance_utils.containment_to_distance (point estimate) and keeps ANIResult.ani:
//     g(c) = 0.0                             if c <= 0.0001
//          = 1.0                             if c >= 0.9999
//          = 1 - (1.0 - pow(c, 1.0 / k))     otherwise (libm pow, as CPython's float ** calls it)
//     ani  = (g(min) + g(max)) / 2.0
// (restated from sourmash's documented behaviour; sourmash is not vendored, so no reference-generated output pins it.)
// The Python float is the TEXT the writer printed: the f32 containment with 6 significant digits (ksp::format_float,
// "%.6g") parsed back.  So g depends on the 6-digit decimal only.  The device cannot call glibc's pow, so it
//   1. computes that decimal exactly with integer arithmetic (the 24-bit mantissa times 10^q fits in 64 bits,
//      rounding half to even on the exact binary value, as printf does: 13/128 = 0.1015625 prints 0.101562), and
//   2. looks g up in a table the host filled with the text definition: one double per decimal d * 10^-q,
//      d in [100000, 999999], q in 6..9 (4 x 900 000 entries, 28.8 MB per k).
// Decimals below 0.0001 (q = 10) and 1 or more map to the constants 0.0 / 1.0; the table's own entries at
// 0.0001 and from 0.9999 up hold those constants too, since they are filled by g.  NaN has no value: an error.
#ifndef KSPIDER_ANI_H
#define KSPIDER_ANI_H
#include <cstdint>

#ifdef __HIPCC__
#define KSP_HD __host__ __device__
#else
#define KSP_HD
#endif

namespace ksp {

constexpr uint32_t kAniDecade = 900000;            // 6-digit mantissas 100000..999999
constexpr uint32_t kAniTableSize = 4 * kAniDecade; // q = 9, 8, 7, 6 (0.0001 .. 0.999999)
constexpr int64_t kAniNaN = -1, kAniZero = -2, kAniOne = -3;

// 6-significant-digit decimal of the f32 containment c as "%.6g" prints it: table index, or kAniNaN / kAniZero / kAniOne
KSP_HD inline int64_t ani_code(const float c) {
    if (c != c) return kAniNaN;
    if (!(c >= 9.0e-5f)) return kAniZero;   // 0, negatives, and every float that prints below 0.0001
    if (c >= 1.0f) return kAniOne;          // 1 and up, inf
    const uint32_t bits = __builtin_bit_cast(uint32_t, c);
    const uint64_t m = (bits & 0x7FFFFFu) | 0x800000u;          // c = m * 2^-s, c normal here
    const int s = 150 - (int)(bits >> 23);                       // 24 .. 37
    uint64_t p10 = 1000000;                                      // 10^q, q = 6 .. 10
    int q = 6;
    while ((m * p10) >> s < 100000) { p10 *= 10; ++q; }          // the first q with c * 10^q >= 10^5 (q <= 10: c >= 9e-5)
    const uint64_t P = m * p10;                                  // < 2^24 * 10^10 < 2^58
    const uint64_t lo = P >> s, rem = P & ((1ull << s) - 1), half = 1ull << (s - 1);
    uint64_t d = lo + ((rem > half || (rem == half && (lo & 1))) ? 1 : 0);
    if (d == 1000000) { d = 100000; --q; }
    if (q >= 10) return kAniZero;
    if (q <= 5) return kAniOne;
    return (int64_t)(9 - q) * kAniDecade + (int64_t)(d - 100000);
}

// g of one containment through the table; false on NaN
KSP_HD inline bool ani_lookup(const float c, const double* __restrict__ table, double* g) {
    const int64_t code = ani_code(c);
    if (code == kAniNaN) return false;
    *g = code == kAniZero ? 0.0 : code == kAniOne ? 1.0 : table[code];
    return true;
}

// average ANI of a row from its two containment floats (columns 3 and 5); false on NaN
KSP_HD inline bool ani_of_row(const float mn, const float mx, const double* __restrict__ table, double* out) {
    double g3, g5;
    if (!ani_lookup(mn, table, &g3) || !ani_lookup(mx, table, &g5)) return false;
    *out = (g3 + g5) / 2.0;
    return true;
}

}  // namespace ksp

#include <memory>
#include <string>
#include <unordered_map>
#include <vector>
namespace ksp {
// g of a containment given as the double a TSV text parses to (the text definition; NaN -> NaN)
double ani_g(double c, int ksize);
// the table of ani_code for k-mer size ksize: built on host threads on first use, cached per k
std::shared_ptr<const std::vector<double>> ani_table(int ksize);
// text of a double as Python's repr() prints it; buf must hold 32 bytes; returns the length
int format_py_repr(char* buf, double v);
// k-mer size of an index: the first line of PREFIX.extra, read as Python's int() reads it (throws)
int read_extra_ksize(const std::string& prefix);
struct EdgeRow;
// float containments of a pairwise row, exactly as the TSV writer computes them (columns 3 and 5)
void row_min_max(uint64_t shared, uint32_t n1, uint32_t n2, float* mn, float* mx);
// PREFIX_kSpider_pairwise.ani_col.tsv for the rows write_pairwise_tsv wrote (same order, same float maths), through
// .partial + rename; throws on a NaN row
void write_ani_column(const std::string& prefix, const std::vector<EdgeRow>& rows,
                      const std::unordered_map<uint32_t, uint32_t>& kmer_count, const double* table, int threads);
}  // namespace ksp
#endif
