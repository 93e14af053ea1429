// The host side of the sketch arithmetic: the threshold of `scaled`, MurmurHash3_x64_128 over any bytes, the hash
// of one k-mer, and ksp_sketch_cpu, the plain single-thread loop over sketch_hash.h.  The loop is the timing baseline of the
// device's hash pass (tools/sketch_times.py) and what the file driver runs with KSPIDER_SKETCH=host.  Host only.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "sketch_hash.h"

namespace sk = ksp_sketch;

namespace {

// bytes 8i .. 8i + 7 of a buffer of `len` bytes as a little-endian word, 0 at and behind len
uint64_t word_at(const uint8_t* p, const uint64_t len, const uint64_t i) {
    uint64_t w = 0;
    const uint64_t at = 8 * i, n = at >= len ? 0 : std::min<uint64_t>(8, len - at);
    for (uint64_t b = 0; b < n; ++b) w |= (uint64_t)p[at + b] << (8 * b);
    return w;
}

// ksp_sketch_cpu and, with counts (out_abund may then be NULL only with capacity 0), ksp_sketch_cpu_abund
int sketch_cpu(const char* who, const bool counted, const uint8_t* seq, const uint64_t n_bytes, const uint64_t* src_offsets, const uint32_t n_sources, const int ksize,
               const uint64_t max_hash, const uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, const uint64_t capacity, uint64_t* out_offsets, uint64_t* needed) {
    if (!out_offsets || !needed || (!out_keys && capacity) || (counted && !out_abund && capacity)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::check_sketch_args(who, seq, n_bytes, src_offsets, n_sources, ksize)) return rc;
    try {
        const unsigned k = (unsigned)ksize;
        std::vector<uint64_t> all, run;
        std::vector<uint32_t> counts;
        out_offsets[0] = 0;
        for (uint32_t s = 0; s < n_sources; ++s) {
            run.clear();
            sk::Kmer fw{0, 0};   // the last min(have, k) bases, right-aligned
            unsigned have = 0;   // bases since the last break, capped at k
            for (uint64_t p = src_offsets[s]; p < src_offsets[s + 1]; ++p) {
                const unsigned c = seq[p];
                if (!sk::is_base(c)) { have = 0; fw = sk::Kmer{0, 0}; continue; }
                fw = sk::shift_left(fw, 2);
                fw.lo |= sk::base_code(c);
                if (have < k) ++have;
                if (have < k) continue;
                const sk::Kmer left = sk::shift_left(fw, 128 - 2 * k);   // (drops the bases older than k)
                const uint64_t h = sk::kmer_hash(sk::canonical(left, k), k, seed);
                if (h <= max_hash) run.push_back(h);
            }
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

}  // namespace

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
