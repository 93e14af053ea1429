// The arithmetic of the protein, dayhoff and hp FracMinHash sketches, one copy for the device kernels
// (sketch_kernels.hip.h) and the host loop (sketch_cpu.cpp): which bytes are residues, the letter a residue is hashed as,
// the codon of a packed k-mer and the letter it translates to, and Murmur over up to 64 letters held as little-endian words.
// What the DNA path calls is in sketch_hash.h and is not touched.
#ifndef KSPIDER_SKETCH_MOL_H
#define KSPIDER_SKETCH_MOL_H
#include "sketch_hash.h"

namespace ksp_sketch {

// is the byte a residue: an ASCII letter of either case, or '*'?
KSP_HD bool is_residue(const unsigned c) {
    const unsigned u = c & 0xDFu;
    return (c < 128 && u >= 'A' && u <= 'Z') || c == '*';
}

// The letter a byte is hashed as for molecule type mol (1 protein, 2 dayhoff, 3 hp); 0 for a byte that is no residue.  The two
// reduced alphabets as one string over A .. Z each:
//   dayhoff  C -> a;  A G P S T -> b;  D E N Q -> c;  H K R -> d;  I L M V -> e;  F W Y -> f;  B J O U X Z -> X
//   hp       A F G I L M P V W Y -> h;  N C S T D E R H K Q -> p;  B J O U X Z -> X
KSP_HD unsigned residue_letter(const int mol, const unsigned c) {
    if (!is_residue(c)) return 0;
    if (c == '*') return '*';
    const unsigned u = c & 0xDFu;
    if (mol == 2) return (unsigned char)"bXaccfbdeXdeecXbcdbbXefXfX"[u - 'A'];
    if (mol == 3) return (unsigned char)"hXppphhphXphhpXhppppXhhXhX"[u - 'A'];
    return u;
}

// The standard genetic code, indexed by 16 b1 + 4 b2 + b3 with T, C, A, G = 0 .. 3.
KSP_HD unsigned genetic_code(const unsigned i) { return (unsigned char)"FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"[i & 63u]; }

// The letter, already encoded for mol, of the codon whose three 2-bit codes (sketch_hash.h: A C G T = 0 .. 3) are the 6 bits of
// `packed`, the first base on top: entry `packed` of the 64-byte table both sides look codons up in.
KSP_HD unsigned codon_letter(const int mol, const unsigned packed) {
    // A C G T = 0 1 2 3  ->  T C A G = 0 1 2 3
    const unsigned b1 = (0x36u >> (2 * ((packed >> 4) & 3u))) & 3u, b2 = (0x36u >> (2 * ((packed >> 2) & 3u))) & 3u, b3 = (0x36u >> (2 * (packed & 3u))) & 3u;
    return residue_letter(mol, genetic_code(16 * b1 + 4 * b2 + b3));
}

// codon j (bases 3j .. 3j + 2) of a left-aligned packed k-mer as 6 bits, 0 <= j <= 20
KSP_HD unsigned codon_at(const Kmer a, const unsigned j) { return (unsigned)(shift_left(a, 6 * j).hi >> 58); }

// the k <= 21 letters a left-aligned packed k-mer of 3k bases translates to, as the little-endian words a hash reads: letter j is
// byte j; table = the 64 letters of codon_letter
template <class Table>
KSP_HD void translate_words(const Kmer a, const unsigned k, const Table table, u64 w[3]) {
    w[0] = w[1] = w[2] = 0;
KSP_UNROLL
    for (unsigned j = 0; j < 21; ++j)
        if (j < k) w[j >> 3] |= (u64)table[codon_at(a, j)] << (8 * (j & 7));
}

// h1 of MurmurHash3_x64_128 over k letters (1 <= k <= 8 * kWords) held as little-endian words; the bytes at and behind k are 0
template <int kWords>
KSP_HD u64 letters_hash(const u64* w, const unsigned k, const u32 seed) {
    Murmur m(seed);
    const unsigned blocks = k >> 4, rem = k & 15;
KSP_UNROLL
    for (unsigned b = 0; b < (kWords + 1) / 2; ++b) {
        const u64 k1 = w[2 * b], k2 = 2 * b + 1 < kWords ? w[2 * b + 1] : 0;
        if (b < blocks) m.block(k1, k2);
        else if (b == blocks) m.tail(k1, k2, rem);
    }
    m.finish(k);
    return m.h1;
}

}  // namespace ksp_sketch
#endif
