// The text of one row of the pairwise TSV, and of one float in it, in integer arithmetic: what tsv.hip runs per record on the
// device.  Plain C++ that compiles for the host as well (tsv_text_check.cpp compares it with libc there), no HIP call.
//
// A float's text is that of snprintf("%.6g", (double)v) = std::ostream << float (ksp::format_float), byte for byte:
//   v = m * 2^e with m < 2^24, exactly.  b = floor(log2 v); X0 = floor(b * log10(2)) is the decimal exponent X (10^X <= v <
//   10^(X+1)) or one below it, because 2^b <= v < 2^(b+1).  With p = 5 - X, v * 10^p = m * 2^e * 10^p lies in [10^5, 10^6): its
//   integer part q is the six significant digits before rounding, and the rest decides the rounding.  Both come from integers:
//     p >= 0:  N = m * 10^p < 2^24 * 10^18 < 2^84 (128-bit product), then q = N >> -e, rest = the bits shifted out, compared
//              with the half 2^(-e-1) (e >= 0: N << e, no rest).
//     p <  0:  v >= 10^6, so e >= -4 and A = m << max(e, 0) < 2^40; D = 10^-p << max(-e, 0) < 2^28; q = A / D, and 2 * (A % D)
//              is compared with D.
//   q >= 10^6 at X0 says, exactly, that v >= 10^(X0+1): then X = X0 + 1 and the digits are taken again.  Round to nearest, a tie
//   (rest == half) to the even q; a q that reaches 10^6 becomes 10^5 with X + 1.  Nothing is ever rounded twice and no
//   floating-point operation takes part, so the six digits are those of the exact binary value, as glibc prints them.
//   Notation by the rules of %g: scientific (d.ddddde[+-]XX) when X < -4 or X >= 6, fixed otherwise; trailing zeros and a
//   bare '.' are dropped.
// Domain: 0, +inf ("inf") and the finite positive floats in [2^-40, 2^40).  A row only produces values in [2^-33, 2^33] (counts
// and sums are below 2^32), 0 and inf.  Everything else — denormals, other magnitudes, negatives (-0 too), NaN — is refused.
//
// Lengths: a float of the domain is at most 11 bytes ("1.23456e-05", "0.000123456"), so a row is at least
// KSP_TSV_ROW_MIN = 12 bytes ("0\t0\t0\t0\t0\t0\n": six fields of one byte, six separators) and at most KSP_TSV_ROW_MAX = 79:
// two ids of 10 digits, a shared count of 20, three floats of 11, six separators.  (82 would need a sign on every float.)
#ifndef KSPIDER_TSV_TEXT_H
#define KSPIDER_TSV_TEXT_H
#include <cstdint>

#ifdef __HIPCC__
#define KSP_TSV_HD __host__ __device__ inline
#else
#define KSP_TSV_HD inline
#endif

#define KSP_TSV_ROW_MIN 12
#define KSP_TSV_ROW_MAX 79
#define KSP_TSV_FLOAT_MAX 11

namespace ksp_tsv {

// the six significant digits of a float of the domain, rounded: value ~ q * 10^(X - 5), 10^5 <= q < 10^6
struct FloatDigits {
    enum Kind : uint32_t { kNumber, kZero, kInf, kRefused };
    uint32_t q;
    int32_t X;
    uint32_t kind;
};

KSP_TSV_HD uint64_t pow10_u64(int k) {   // k <= 19
    uint64_t r = 1;
    for (int i = 0; i < k; ++i) r *= 10;
    return r;
}

// floor(v * 10^p) and how the rest compares with one half (-1 below, 0 a tie, 1 above); v = m * 2^e
KSP_TSV_HD uint64_t scaled_digits(const uint32_t m, const int e, const int p, int* rest) {
    if (p >= 0) {
        const unsigned __int128 N = (unsigned __int128)m * pow10_u64(p);
        if (e >= 0) { *rest = -1; return (uint64_t)(N << e); }
        const int s = -e;   // 1 .. 63
        const uint64_t low = (uint64_t)N & ((1ull << s) - 1), half = 1ull << (s - 1);
        *rest = low < half ? -1 : low == half ? 0 : 1;
        return (uint64_t)(N >> s);
    }
    const uint64_t A = e >= 0 ? (uint64_t)m << e : (uint64_t)m;
    const uint64_t D = pow10_u64(-p) << (e < 0 ? -e : 0);
    const uint64_t q = A / D, r2 = 2 * (A % D);
    *rest = r2 < D ? -1 : r2 == D ? 0 : 1;
    return q;
}

KSP_TSV_HD FloatDigits float_digits(const uint32_t bits) {
    FloatDigits f{0, 0, FloatDigits::kRefused};
    if (bits == 0) { f.kind = FloatDigits::kZero; return f; }
    if (bits == 0x7F800000u) { f.kind = FloatDigits::kInf; return f; }
    const int b = (int)(bits >> 23) - 127;         // (a set sign bit makes this >= 129: refused)
    if (b < -40 || b > 39) return f;               // denormals, NaN, negatives and the magnitudes outside [2^-40, 2^40)
    const uint32_t m = (bits & 0x7FFFFFu) | 0x800000u;
    const int e = b - 23;
    int X = (b * 1233) >> 12;                      // floor(b * log10(2)) for |b| <= 40 (tsv_text_check.cpp checks every b)
    int rest = 0;
    uint64_t q = scaled_digits(m, e, 5 - X, &rest);
    if (q >= 1000000u) { ++X; q = scaled_digits(m, e, 5 - X, &rest); }
    if (rest > 0 || (rest == 0 && (q & 1))) ++q;   // to nearest, a tie to even
    if (q == 1000000u) { q = 100000u; ++X; }
    f.q = (uint32_t)q;
    f.X = X;
    f.kind = FloatDigits::kNumber;
    return f;
}

KSP_TSV_HD int n_digits(const uint64_t v) {
    int n = 1;
    for (uint64_t p = 10; n < 20 && v >= p; p *= 10) ++n;
    return n;
}

// Where the text goes.  Both sinks take the same calls, so the length that is counted is the length that is written.
struct Counter {
    uint32_t n = 0;
    KSP_TSV_HD void put(char) { ++n; }
    KSP_TSV_HD void digits(uint64_t, const int count) { n += (uint32_t)count; }
};
struct Writer {
    char* p;
    KSP_TSV_HD void put(const char c) { *p++ = c; }
    // `count` decimal digits of v, zero-padded on the left, written from the last digit back
    KSP_TSV_HD void digits(uint64_t v, const int count) {
        int k = count;
        while (k > 0 && (v >> 32)) { p[--k] = (char)('0' + (int)(v % 10)); v /= 10; }
        uint32_t w = (uint32_t)v;
        while (k > 0) { p[--k] = (char)('0' + (int)(w % 10)); w /= 10; }
        p += count;
    }
};

template <class Out>
KSP_TSV_HD void emit_uint(Out& o, const uint64_t v) { o.digits(v, n_digits(v)); }

template <class Out>
KSP_TSV_HD void emit_float(Out& o, const FloatDigits& f) {
    if (f.kind == FloatDigits::kZero) { o.put('0'); return; }
    if (f.kind == FloatDigits::kInf) { o.put('i'); o.put('n'); o.put('f'); return; }
    if (f.kind != FloatDigits::kNumber) return;
    uint32_t q = f.q;
    int nd = 6;
    while (nd > 1 && q % 10 == 0) { q /= 10; --nd; }   // q: the nd digits that are left without the trailing zeros
    const int X = f.X;
    if (X < -4 || X >= 6) {
        const uint32_t lead = (uint32_t)pow10_u64(nd - 1);
        o.digits(q / lead, 1);
        if (nd > 1) { o.put('.'); o.digits(q % lead, nd - 1); }
        o.put('e');
        o.put(X < 0 ? '-' : '+');
        o.digits((uint64_t)(X < 0 ? -X : X), 2);
    } else if (X >= 0) {
        const int ip = X + 1;   // digits before the point
        if (nd <= ip) o.digits((uint64_t)q * pow10_u64(ip - nd), ip);
        else {
            const uint32_t cut = (uint32_t)pow10_u64(nd - ip);
            o.digits(q / cut, ip);
            o.put('.');
            o.digits(q % cut, nd - ip);
        }
    } else {
        o.put('0');
        o.put('.');
        o.digits(0, -X - 1);
        o.digits(q, nd);
    }
}

// min, avg and max containment of a row: the single-precision maths of the pairwise writer (index_io.cpp format_rows)
struct RowText {
    uint32_t id1, id2;
    uint64_t shared;
    FloatDigits col[3];
};

// id1 \t id2 \t shared \t min \t avg \t max \n
template <class Out>
KSP_TSV_HD void emit_row(Out& o, const RowText& r) {
    emit_uint(o, r.id1);
    o.put('\t');
    emit_uint(o, r.id2);
    o.put('\t');
    emit_uint(o, r.shared);
    for (int c = 0; c < 3; ++c) {
        o.put('\t');
        emit_float(o, r.col[c]);
    }
    o.put('\n');
}

}  // namespace ksp_tsv
#endif
