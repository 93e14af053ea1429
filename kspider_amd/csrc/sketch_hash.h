// The arithmetic of a DNA FracMinHash sketch, one copy for the device kernels (sketch_kernels.hip.h) and the host loop
// (sketch_cpu.cpp): the 2-bit code of a base, the reverse complement of a packed k-mer, the ASCII text of a packed k-mer, and
// the first word of MurmurHash3_x64_128 over it.
//
// A packed k-mer (1 <= k <= 64) is 128 bits (hi, lo), LEFT-ALIGNED and big-endian: base j of the k-mer is the 2-bit group at
// bits 127 - 2j .. 126 - 2j, everything below the 2k-th bit from the top is 0.  The codes are A < C < G < T = 0 .. 3, which is
// the order of the letters, so comparing two packed k-mers of the same k as 128-bit numbers compares their upper-case texts.
#ifndef KSPIDER_SKETCH_HASH_H
#define KSPIDER_SKETCH_HASH_H
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define KSP_HD __host__ __device__ inline
#define KSP_UNROLL _Pragma("unroll")
#else
#define KSP_HD inline
#define KSP_UNROLL
#endif

namespace ksp_sketch {

typedef uint64_t u64;
typedef uint32_t u32;

struct Kmer {
    u64 hi, lo;
};

// is the byte one of ACGTacgt?
KSP_HD bool is_base(const unsigned c) {
    const unsigned u = c & 0xDFu;   // lower case -> upper case
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
// the code of a base byte (anything for another byte): bits 2..1 of A C G T are 0 1 3 2
KSP_HD unsigned base_code(const unsigned c) {
    const unsigned x = (c >> 1) & 3u;
    return x ^ (x >> 1);
}

// the 32 two-bit groups of a word in reverse order
KSP_HD u64 reverse_groups(u64 x) {
#if defined(__HIP_DEVICE_COMPILE__)
    x = __brevll(x);   // every bit reversed: the groups are in place, the two bits of each swapped
    return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
#else
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}

// (hi, lo) << s for 0 <= s <= 127
KSP_HD Kmer shift_left(const Kmer a, const unsigned s) {
    if (s == 0) return a;
    if (s >= 64) return Kmer{a.lo << (s - 64), 0};
    return Kmer{(a.hi << s) | (a.lo >> (64 - s)), a.lo << s};
}

// a word whose top 2k bits are kept: the bits of a left-aligned k-mer
KSP_HD Kmer keep_top(const Kmer a, const unsigned k) {
    if (k >= 64) return a;
    if (k > 32) return Kmer{a.hi, a.lo & ~(~0ull >> (2 * (k - 32)))};
    return Kmer{k == 32 ? a.hi : a.hi & ~(~0ull >> (2 * k)), 0};
}

// the reverse complement of a left-aligned k-mer, left-aligned: the groups reversed over all 128 bits (the k-mer ends up
// right-aligned), complemented (A <-> T, C <-> G is 3 - code), and shifted back up, which drops the complemented padding
KSP_HD Kmer reverse_complement(const Kmer a, const unsigned k) {
    const Kmer r{~reverse_groups(a.lo), ~reverse_groups(a.hi)};
    return shift_left(r, 128 - 2 * k);
}

KSP_HD bool less_than(const Kmer a, const Kmer b) { return a.hi != b.hi ? a.hi < b.hi : a.lo < b.lo; }

KSP_HD Kmer canonical(const Kmer fw, const unsigned k) {
    const Kmer rc = reverse_complement(fw, k);
    return less_than(rc, fw) ? rc : fw;
}

// bases 8i .. 8i + 7 of a left-aligned k-mer as 16 bits, the first of them on top (0 <= i <= 7)
KSP_HD u32 chunk_of(const Kmer a, const unsigned i) { return (u32)(((i < 4 ? a.hi : a.lo) >> (48 - 16 * (i & 3))) & 0xFFFFu); }

// the ASCII text of 8 packed bases as the little-endian word a hash reads from memory: the first base is the lowest byte
KSP_HD u64 ascii_of(const u32 chunk) {
    u64 out = 0;
KSP_UNROLL
    for (int j = 0; j < 8; ++j) {
        const u32 code = (chunk >> (14 - 2 * j)) & 3u;
        out |= (u64)((0x54474341u >> (8 * code)) & 0xFFu) << (8 * j);   // "ACGT"[code]
    }
    return out;
}

KSP_HD u64 rotl64(const u64 x, const int r) { return (x << r) | (x >> (64 - r)); }
KSP_HD u64 fmix64(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// MurmurHash3_x64_128 (Austin Appleby, public domain) over `len` bytes that a reader hands out as little-endian 64-bit words:
// word(i) = bytes 8i .. 8i + 7, bytes at and behind `len` read as 0.  The body takes the 16-byte blocks; the tail's 15 cases
// (1 .. 15 bytes left: the byte-by-byte switch of the original) are the two words behind the blocks, which the zero padding
// makes equal to what the switch assembles; then the finaliser.  h[0], h[1] = the two result words.
struct Murmur {
    u64 h1, h2;
    KSP_HD explicit Murmur(const u32 seed) : h1(seed), h2(seed) {}
    KSP_HD static u64 mix1(u64 k1) { k1 *= 0x87c37b91114253d5ull; k1 = rotl64(k1, 31); return k1 * 0x4cf5ad432745937full; }
    KSP_HD static u64 mix2(u64 k2) { k2 *= 0x4cf5ad432745937full; k2 = rotl64(k2, 33); return k2 * 0x87c37b91114253d5ull; }
    KSP_HD void block(const u64 k1, const u64 k2) {
        h1 ^= mix1(k1);
        h1 = rotl64(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52dce729;
        h2 ^= mix2(k2);
        h2 = rotl64(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495ab5;
    }
    // the words behind the last block; rem = len & 15 bytes are left
    KSP_HD void tail(const u64 k1, const u64 k2, const unsigned rem) {
        if (rem > 8) h2 ^= mix2(k2);
        if (rem > 0) h1 ^= mix1(k1);
    }
    KSP_HD void finish(const u64 len) {
        h1 ^= len; h2 ^= len;
        h1 += h2; h2 += h1;
        h1 = fmix64(h1); h2 = fmix64(h2);
        h1 += h2; h2 += h1;
    }
};

// the low n bytes of a word (0 <= n <= 8)
KSP_HD u64 low_bytes(const u64 w, const unsigned n) { return n >= 8 ? w : w & ((1ull << (8 * n)) - 1); }

// h1 of MurmurHash3_x64_128 over the k ASCII letters of a left-aligned packed k-mer
KSP_HD u64 kmer_hash(const Kmer a, const unsigned k, const u32 seed) {
    Murmur m(seed);
    const unsigned blocks = k >> 4, rem = k & 15;
KSP_UNROLL
    for (unsigned b = 0; b < 4; ++b)
        if (b < blocks) m.block(ascii_of(chunk_of(a, 2 * b)), ascii_of(chunk_of(a, 2 * b + 1)));
    if (rem) {   // (blocks <= 3 here: the chunks exist)
        const u64 k1 = low_bytes(ascii_of(chunk_of(a, 2 * blocks)), rem);
        const u64 k2 = rem > 8 ? low_bytes(ascii_of(chunk_of(a, 2 * blocks + 1)), rem - 8) : 0;
        m.tail(k1, k2, rem);
    }
    m.finish(k);
    return m.h1;
}

}  // namespace ksp_sketch
#endif
