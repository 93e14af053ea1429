// The host side of the sketch arithmetic: the threshold of `scaled`, MurmurHash3_x64_128 over any bytes, the hash
// of one k-mer, and ksp_sketch_cpu, the plain single-thread loop over sketch_hash.h.  The loop is the timing baseline of the
// device's hash pass (tools/sketch_times.py) and what the file driver runs with KSPIDER_SKETCH=host.  ksp_sketch_cpu_mol is the
// same for the protein, dayhoff and hp molecule types over sketch_mol.h.  sketch_cpu_frame is what every loop
// shares from the kept hashes on; each_base_window rolls the bases for the DNA loop (k bases) and the translated one (3k).  Host only.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "sketch_hash.h"
#include "sketch_mol.h"
#include "sketch_windows.h"

namespace sk = ksp_sketch;

namespace {

// bytes 8i .. 8i + 7 of a buffer of `len` bytes as a little-endian word, 0 at and behind len
uint64_t word_at(const uint8_t* p, const uint64_t len, const uint64_t i) {
    uint64_t w = 0;
    const uint64_t at = 8 * i, n = at >= len ? 0 : std::min<uint64_t>(8, len - at);
    for (uint64_t b = 0; b < n; ++b) w |= (uint64_t)p[at + b] << (8 * b);
    return w;
}

// The frame of the host loops: kept_of(first, last, run) appends the kept hashes, repeats included, of the source that is the
// bytes [first, last); the rest — order, counts, bounds, the overflow rule — is the same for every molecule type.
// counted: out_abund may then be NULL only with capacity 0.
template <class KeptOf>
int sketch_cpu_frame(const char* who, const bool counted, const uint8_t* seq, const uint64_t n_bytes, const uint64_t* src_offsets, const uint32_t n_sources, const int ksize,
                     uint64_t* out_keys, uint32_t* out_abund, const uint64_t capacity, uint64_t* out_offsets, uint64_t* needed, KeptOf kept_of) {
    if (!out_offsets || !needed || (!out_keys && capacity) || (counted && !out_abund && capacity)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::check_sketch_args(who, seq, n_bytes, src_offsets, n_sources, ksize)) return rc;
    try {
        std::vector<uint64_t> all, run;
        std::vector<uint32_t> counts;
        out_offsets[0] = 0;
        for (uint32_t s = 0; s < n_sources; ++s) {
            run.clear();
            kept_of(src_offsets[s], src_offsets[s + 1], run);
            std::sort(run.begin(), run.end());
            if (counted)
                for (size_t i = 0, j = 0; i < run.size(); i = j) {   // the length of every run of equal hashes
                    while (j < run.size() && run[j] == run[i]) ++j;
                    counts.push_back((uint32_t)std::min<uint64_t>(j - i, 0xFFFFFFFFull));
                }
            run.erase(std::unique(run.begin(), run.end()), run.end());
            all.insert(all.end(), run.begin(), run.end());
            out_offsets[s + 1] = all.size();
        }
        *needed = all.size();
        if (all.size() > capacity) {
            ksp::set_error(std::string(who) + ": " + std::to_string(all.size()) + " keys, room for " + std::to_string(capacity));
            return KSP_E_OVERFLOW;
        }
        if (!all.empty()) std::memcpy(out_keys, all.data(), 8 * all.size());
        if (counted && !counts.empty()) std::memcpy(out_abund, counts.data(), 4 * counts.size());
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
}

using sk::each_base_window;   // (sketch_windows.h: the rolling window of the DNA loops)

// ksp_sketch_cpu and, with counts, ksp_sketch_cpu_abund: every window of k bases, canonical form, hashed
int sketch_cpu(const char* who, const bool counted, const uint8_t* seq, const uint64_t n_bytes, const uint64_t* src_offsets, const uint32_t n_sources, const int ksize,
               const uint64_t max_hash, const uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, const uint64_t capacity, uint64_t* out_offsets, uint64_t* needed) {
    const unsigned k = (unsigned)ksize;
    return sketch_cpu_frame(who, counted, seq, n_bytes, src_offsets, n_sources, ksize, out_keys, out_abund, capacity, out_offsets, needed,
                            [&](const uint64_t first, const uint64_t last, std::vector<uint64_t>& run) {
                                each_base_window(seq, first, last, k, [&](const sk::Kmer& left) {
                                    const uint64_t h = sk::kmer_hash(sk::canonical(left, k), k, seed);
                                    if (h <= max_hash) run.push_back(h);
                                });
                            });
}

// protein input: every window of k residue bytes, its letters packed into words and hashed
int sketch_cpu_protein(const char* who, const bool counted, const uint8_t* seq, const uint64_t n_bytes, const uint64_t* src_offsets, const uint32_t n_sources, const int ksize,
                       const int mol, const uint64_t max_hash, const uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, const uint64_t capacity, uint64_t* out_offsets,
                       uint64_t* needed) {
    const unsigned k = (unsigned)ksize;
    uint8_t letter_of[256];
    for (unsigned c = 0; c < 256; ++c) letter_of[c] = (uint8_t)sk::residue_letter(mol, c);
    return sketch_cpu_frame(who, counted, seq, n_bytes, src_offsets, n_sources, ksize, out_keys, out_abund, capacity, out_offsets, needed,
                            [&](const uint64_t first, const uint64_t last, std::vector<uint64_t>& run) {
                                uint64_t have = 0;   // residues since the last break
                                for (uint64_t p = first; p < last; ++p) {
                                    if (!letter_of[seq[p]]) { have = 0; continue; }
                                    if (++have < k) continue;
                                    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                                    const uint8_t* at = seq + (p + 1 - k);
                                    for (unsigned j = 0; j < k; ++j) w[j >> 3] |= (uint64_t)letter_of[at[j]] << (8 * (j & 7));
                                    const uint64_t h = sk::letters_hash<8>(w, k, seed);
                                    if (h <= max_hash) run.push_back(h);
                                }
                            });
}

// translated input: every window of 3k bases, both strands translated and hashed
int sketch_cpu_translated(const char* who, const bool counted, const uint8_t* seq, const uint64_t n_bytes, const uint64_t* src_offsets, const uint32_t n_sources, const int ksize,
                          const int mol, const uint64_t max_hash, const uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, const uint64_t capacity, uint64_t* out_offsets,
                          uint64_t* needed) {
    const unsigned k = (unsigned)ksize, k3 = 3 * k;
    uint8_t codon[64];
    for (unsigned c = 0; c < 64; ++c) codon[c] = (uint8_t)sk::codon_letter(mol, c);
    return sketch_cpu_frame(who, counted, seq, n_bytes, src_offsets, n_sources, ksize, out_keys, out_abund, capacity, out_offsets, needed,
                            [&](const uint64_t first, const uint64_t last, std::vector<uint64_t>& run) {
                                each_base_window(seq, first, last, k3, [&](const sk::Kmer& left) {
                                    uint64_t w[3];
                                    sk::translate_words(left, k, codon, w);
                                    const uint64_t h_f = sk::letters_hash<3>(w, k, seed);
                                    sk::translate_words(sk::reverse_complement(left, k3), k, codon, w);
                                    const uint64_t h_r = sk::letters_hash<3>(w, k, seed);
                                    if (h_f <= max_hash) run.push_back(h_f);
                                    if (h_r <= max_hash) run.push_back(h_r);
                                });
                            });
}

}  // namespace

int ksp::check_sketch_mol(const char* who, const int ksize, const int moltype, const uint64_t flags) {
    if (moltype < KSP_MOL_DNA || moltype > KSP_MOL_HP) { set_error(std::string(who) + ": moltype is 0 (DNA), 1 (protein), 2 (dayhoff) or 3 (hp)"); return KSP_E_ARG; }
    if (flags & ~KSP_SKETCH_TRANSLATE) { set_error(std::string(who) + ": flags is 0 or KSP_SKETCH_TRANSLATE"); return KSP_E_ARG; }
    if (!flags) return KSP_OK;   // (ksize 1 .. 64: check_sketch_args)
    if (moltype == KSP_MOL_DNA) { set_error(std::string(who) + ": KSP_SKETCH_TRANSLATE takes a protein, dayhoff or hp moltype"); return KSP_E_ARG; }
    if (ksize < 1 || ksize > 21) { set_error(std::string(who) + ": ksize is 1 .. 21 with KSP_SKETCH_TRANSLATE (3 * ksize <= 63 bases)"); return KSP_E_ARG; }
    return KSP_OK;
}

int ksp::check_sketch_args(const char* who, const void* seq, const uint64_t n_bytes, const uint64_t* off, const uint32_t n_sources, const int ksize) {
    if (!off || (!seq && n_bytes)) { set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (ksize < 1 || ksize > 64) { set_error(std::string(who) + ": ksize is 1 .. 64"); return KSP_E_ARG; }
    if (n_sources == 0) { set_error(std::string(who) + ": no source"); return KSP_E_ARG; }
    if (off[0] != 0) { set_error(std::string(who) + ": the source offsets do not start at 0"); return KSP_E_ARG; }
    for (uint32_t s = 0; s < n_sources; ++s)
        if (off[s + 1] < off[s]) { set_error(std::string(who) + ": the source offsets decrease at source " + std::to_string(s)); return KSP_E_ARG; }
    if (off[n_sources] != n_bytes) { set_error(std::string(who) + ": the source offsets do not end at n_bytes"); return KSP_E_ARG; }
    return KSP_OK;
}

extern "C" int ksp_sketch_max_hash(uint64_t scaled, uint64_t* out) {
    if (!out) { ksp::set_error("ksp_sketch_max_hash: NULL argument"); return KSP_E_ARG; }
    if (scaled == 0) { ksp::set_error("ksp_sketch_max_hash: scaled is 1 or more"); return KSP_E_ARG; }
    *out = scaled == 1 ? ~0ull : (uint64_t)(18446744073709551616.0 / (double)scaled);
    return KSP_OK;
}

extern "C" int ksp_murmur64(const void* data, uint64_t len, uint32_t seed, uint64_t out[2]) {
    if (!out || (!data && len)) { ksp::set_error("ksp_murmur64: NULL argument"); return KSP_E_ARG; }
    const uint8_t* p = (const uint8_t*)data;
    sk::Murmur m(seed);
    const uint64_t blocks = len / 16;
    for (uint64_t b = 0; b < blocks; ++b) m.block(word_at(p, len, 2 * b), word_at(p, len, 2 * b + 1));
    m.tail(word_at(p, len, 2 * blocks), word_at(p, len, 2 * blocks + 1), (unsigned)(len & 15));
    m.finish(len);
    out[0] = m.h1;
    out[1] = m.h2;
    return KSP_OK;
}

extern "C" int ksp_sketch_kmer_hash(const char* text, int ksize, uint32_t seed, uint64_t* hash, int* valid) {
    if (!text || !hash || !valid) { ksp::set_error("ksp_sketch_kmer_hash: NULL argument"); return KSP_E_ARG; }
    if (ksize < 1 || ksize > 64) { ksp::set_error("ksp_sketch_kmer_hash: ksize is 1 .. 64"); return KSP_E_ARG; }
    *hash = 0;
    *valid = 0;
    sk::Kmer fw{0, 0};
    for (int j = 0; j < ksize; ++j) {
        const unsigned c = (unsigned char)text[j];
        if (!sk::is_base(c)) return KSP_OK;
        const sk::Kmer one = sk::shift_left(sk::Kmer{0, sk::base_code(c)}, 126 - 2 * (unsigned)j);
        fw.hi |= one.hi;
        fw.lo |= one.lo;
    }
    *hash = sk::kmer_hash(sk::canonical(fw, (unsigned)ksize), (unsigned)ksize, seed);
    *valid = 1;
    return KSP_OK;
}

extern "C" int ksp_sketch_cpu(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, uint64_t max_hash,
                              uint32_t seed, uint64_t* out_keys, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed) {
    return sketch_cpu("ksp_sketch_cpu", false, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, nullptr, capacity, out_offsets, needed);
}

extern "C" int ksp_sketch_cpu_abund(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, uint64_t max_hash,
                                    uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed) {
    return sketch_cpu("ksp_sketch_cpu_abund", true, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, out_abund, capacity, out_offsets, needed);
}

extern "C" int ksp_sketch_text_hash(const char* text, int len, int moltype, uint32_t seed, uint64_t* hash, int* valid) {
    const char* who = "ksp_sketch_text_hash";
    if (!text || !hash || !valid) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (len < 1 || len > 64) { ksp::set_error(std::string(who) + ": len is 1 .. 64"); return KSP_E_ARG; }
    if (moltype < KSP_MOL_PROTEIN || moltype > KSP_MOL_HP) { ksp::set_error(std::string(who) + ": moltype is 1 (protein), 2 (dayhoff) or 3 (hp)"); return KSP_E_ARG; }
    *hash = 0;
    *valid = 0;
    uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < len; ++j) {
        const unsigned l = sk::residue_letter(moltype, (unsigned char)text[j]);
        if (!l) return KSP_OK;
        w[j >> 3] |= (uint64_t)l << (8 * (j & 7));
    }
    *hash = sk::letters_hash<8>(w, (unsigned)len, seed);
    *valid = 1;
    return KSP_OK;
}

extern "C" int ksp_sketch_cpu_mol(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, int moltype, uint64_t flags,
                                  uint64_t max_hash, uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed) {
    const char* who = "ksp_sketch_cpu_mol";
    if (const int rc = ksp::check_sketch_mol(who, ksize, moltype, flags)) return rc;
    const bool counted = out_abund != nullptr;
    if (moltype == KSP_MOL_DNA) return sketch_cpu(who, counted, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, out_abund, capacity, out_offsets, needed);
    return (flags & KSP_SKETCH_TRANSLATE ? sketch_cpu_translated : sketch_cpu_protein)(who, counted, seq, n_bytes, src_offsets, n_sources, ksize, moltype, max_hash, seed, out_keys,
                                                                                        out_abund, capacity, out_offsets, needed);
}
