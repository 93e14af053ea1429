// The host side of classify: the argument checks every classify call shares, and ClassifyCpu, the plain
// single-thread form of the session over sketch_hash.h — the timing baseline of the device path (tools/classify_times.py), what
// ksp_classify_cpu is one batch of, and what the file driver runs with KSPIDER_CLASSIFY=host.  It takes the steps the device
// takes, with the same intermediate values: a table of the distinct reference hashes with their holders, one hit word
// (record << 32) | table_index per kept window that hits, sort and unique of the words, the words expanded into
// (record << 32) | reference per holder, sort, run lengths, the cut at min_hits, the summary.  Host only.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "sketch_hash.h"
#include "sketch_windows.h"

namespace sk = ksp_sketch;

int ksp::check_classify_refs(const char* who, const int ksize, const uint64_t* ref_keys, const uint64_t* ref_offsets, const uint32_t n_refs) {
    if (!ref_offsets) { set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (ksize < 1 || ksize > 64) { set_error(std::string(who) + ": ksize is 1 .. 64"); return KSP_E_ARG; }
    if (ref_offsets[0] != 0) { set_error(std::string(who) + ": the reference offsets do not start at 0"); return KSP_E_ARG; }
    for (uint32_t q = 0; q < n_refs; ++q)
        if (ref_offsets[q + 1] < ref_offsets[q]) { set_error(std::string(who) + ": the reference offsets decrease at reference " + std::to_string(q)); return KSP_E_ARG; }
    if (!ref_keys && ref_offsets[n_refs]) { set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    for (uint32_t q = 0; q < n_refs; ++q)
        for (uint64_t i = ref_offsets[q] + 1; i < ref_offsets[q + 1]; ++i)
            if (ref_keys[i] <= ref_keys[i - 1]) { set_error(std::string(who) + ": reference " + std::to_string(q) + " is not strictly ascending"); return KSP_E_ARG; }
    return KSP_OK;
}

int ksp::check_classify_batch(const char* who, const void* seq, const uint64_t n_bytes, const uint64_t* seg_offsets, const uint32_t* seg_records, const uint32_t n_segments) {
    if (!seg_offsets || (!seq && n_bytes)) { set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_segments == 0) { set_error(std::string(who) + ": no record"); return KSP_E_ARG; }
    if (seg_offsets[0] != 0) { set_error(std::string(who) + ": the record offsets do not start at 0"); return KSP_E_ARG; }
    for (uint32_t s = 0; s < n_segments; ++s)
        if (seg_offsets[s + 1] < seg_offsets[s]) { set_error(std::string(who) + ": the record offsets decrease at " + std::to_string(s)); return KSP_E_ARG; }
    if (seg_offsets[n_segments] != n_bytes) { set_error(std::string(who) + ": the record offsets do not end at n_bytes"); return KSP_E_ARG; }
    if (seg_records)
        for (uint32_t s = 0; s < n_segments; ++s)
            if (seg_records[s] == 0xFFFFFFFFu) { set_error(std::string(who) + ": a record id of 2^32 - 1"); return KSP_E_ARG; }
    return KSP_OK;
}

int ksp::check_classify_out(const char* who, const uint32_t min_hits, const void* rows, const void* n_rows, const void* kept_windows, const void* matched,
                            const void* n_refs_hit, const void* best_ref, const void* best_hits, const void* second_hits) {
    if (!rows || !n_rows || !kept_windows || !matched || !n_refs_hit || !best_ref || !best_hits || !second_hits) { set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (min_hits == 0) { set_error(std::string(who) + ": min_hits is 1 or more"); return KSP_E_ARG; }
    return KSP_OK;
}

struct ksp::ClassifyCpu::State {
    unsigned k = 0;
    uint64_t max_hash = 0;
    uint32_t seed = 0;
    // the table: the distinct reference hashes <= max_hash, ascending, and the references that hold each, ascending
    std::vector<uint64_t> tk;
    std::vector<uint32_t> toff, tq;
    std::vector<uint64_t> words;          // (record << 32) | table_index of every kept window that hits
    std::vector<uint32_t> kept_windows;   // per record met so far
    ksp_classify_stats st;
    bool finished = false;
};

ksp::ClassifyCpu::~ClassifyCpu() { delete s_; }

int ksp::ClassifyCpu::open(const char* who, const int ksize, const uint64_t max_hash, const uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets,
                           const uint32_t n_refs) {
    try {
        delete s_;
        s_ = nullptr;
        s_ = new State;
        State& S = *s_;
        std::memset(&S.st, 0, sizeof S.st);
        S.k = (unsigned)ksize;
        S.max_hash = max_hash;
        S.seed = seed;
        std::vector<std::pair<uint64_t, uint32_t>> all;
        for (uint32_t q = 0; q < n_refs; ++q)
            for (uint64_t i = ref_offsets[q]; i < ref_offsets[q + 1]; ++i)
                if (ref_keys[i] <= max_hash) all.emplace_back(ref_keys[i], q);
        if (all.size() >= (1ull << 31)) { set_error(std::string(who) + ": the references hold 2^31 entries or more"); return KSP_E_LIMIT; }
        std::sort(all.begin(), all.end());
        for (size_t i = 0; i < all.size(); ++i) {
            if (i == 0 || all[i].first != all[i - 1].first) { S.tk.push_back(all[i].first); S.toff.push_back((uint32_t)S.tq.size()); }
            S.tq.push_back(all[i].second);   // (a run is strictly ascending: no reference holds a hash twice)
        }
        S.toff.push_back((uint32_t)S.tq.size());
        S.st.table_keys = S.tk.size();
        S.st.table_holders = S.tq.size();
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
}

int ksp::ClassifyCpu::add(const char* who, const uint8_t* seq, const uint64_t* seg_offsets, const uint32_t* seg_records, const uint32_t n_segments) {
    State& S = *s_;
    if (S.finished) { set_error(std::string(who) + ": the session is finished"); return KSP_E_ARG; }
    try {
        for (uint32_t s = 0; s < n_segments; ++s) {
            const uint32_t rec = seg_records ? seg_records[s] : s;
            if (rec >= S.kept_windows.size()) S.kept_windows.resize((size_t)rec + 1, 0);
            uint64_t bases = 0;
            for (uint64_t p = seg_offsets[s]; p < seg_offsets[s + 1]; ++p) bases += sk::is_base(seq[p]);
            S.st.bases += bases;
            sk::each_base_window(seq, seg_offsets[s], seg_offsets[s + 1], S.k, [&](const sk::Kmer& left) {
                ++S.st.valid_kmers;
                const uint64_t h = sk::kmer_hash(sk::canonical(left, S.k), S.k, S.seed);
                if (h > S.max_hash) return;
                ++S.kept_windows[rec];
                ++S.st.kept_windows;
                const auto it = std::lower_bound(S.tk.begin(), S.tk.end(), h);
                if (it != S.tk.end() && *it == h) S.words.push_back(((uint64_t)rec << 32) | (uint64_t)(it - S.tk.begin()));
            });
        }
        ++S.st.batches;
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
}

int ksp::ClassifyCpu::finish(const char* who, const uint32_t n_records, const uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows, uint32_t* kept_windows,
                             uint32_t* matched, uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits, ksp_classify_stats* stats) {
    State& S = *s_;
    if (S.finished) { set_error(std::string(who) + ": the session is finished"); return KSP_E_ARG; }
    if (S.kept_windows.size() > n_records) { set_error(std::string(who) + ": n_records is not above every record id that was added"); return KSP_E_ARG; }
    try {
        S.st.hit_words = S.words.size();
        std::sort(S.words.begin(), S.words.end());
        S.words.erase(std::unique(S.words.begin(), S.words.end()), S.words.end());
        S.st.hit_words_unique = S.words.size();
        std::vector<uint64_t> pairs;   // (record << 32) | reference, one per holder of every distinct hit
        for (const uint64_t w : S.words)
            for (uint32_t j = S.toff[(uint32_t)w]; j < S.toff[(uint32_t)w + 1]; ++j) pairs.push_back((w & 0xFFFFFFFF00000000ull) | S.tq[j]);
        std::sort(pairs.begin(), pairs.end());
        std::vector<ksp_classify_row> out;
        for (size_t i = 0, j = 0; i < pairs.size(); i = j) {
            while (j < pairs.size() && pairs[j] == pairs[i]) ++j;
            if (j - i >= min_hits) out.push_back(ksp_classify_row{(uint32_t)(pairs[i] >> 32), (uint32_t)pairs[i], (uint32_t)(j - i), 0});
        }
        ksp_classify_row* r = (ksp_classify_row*)std::malloc(std::max<size_t>(out.size(), 1) * sizeof(ksp_classify_row));
        if (!r) throw std::bad_alloc();
        if (!out.empty()) std::memcpy(r, out.data(), out.size() * sizeof(ksp_classify_row));
        for (uint32_t i = 0; i < n_records; ++i) {
            kept_windows[i] = i < S.kept_windows.size() ? S.kept_windows[i] : 0;
            matched[i] = n_refs_hit[i] = best_hits[i] = second_hits[i] = 0;
            best_ref[i] = 0xFFFFFFFFu;
        }
        for (const uint64_t w : S.words) ++matched[w >> 32];
        for (const ksp_classify_row& x : out) {   // by (record, reference): a tie keeps the smaller reference
            ++n_refs_hit[x.record];
            if (x.hits > best_hits[x.record]) {
                second_hits[x.record] = best_hits[x.record];
                best_hits[x.record] = x.hits;
                best_ref[x.record] = x.reference;
            } else if (x.hits > second_hits[x.record]) {
                second_hits[x.record] = x.hits;
            }
        }
        S.st.rows = out.size();
        *rows = r;
        *n_rows = out.size();
        if (stats) *stats = S.st;
        S.finished = true;
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
}

extern "C" int ksp_classify_cpu(const uint8_t* seq, uint64_t n_bytes, const uint64_t* rec_offsets, uint32_t n_records, int ksize, uint64_t max_hash, uint32_t seed,
                                const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs, uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows,
                                uint32_t* kept_windows, uint32_t* matched, uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits,
                                ksp_classify_stats* stats) {
    const char* who = "ksp_classify_cpu";
    int rc = KSP_OK;
    if ((rc = ksp::check_classify_out(who, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits))) return rc;
    if ((rc = ksp::check_classify_refs(who, ksize, ref_keys, ref_offsets, n_refs))) return rc;
    if ((rc = ksp::check_classify_batch(who, seq, n_bytes, rec_offsets, nullptr, n_records))) return rc;
    ksp::ClassifyCpu c;
    if ((rc = c.open(who, ksize, max_hash, seed, ref_keys, ref_offsets, n_refs))) return rc;
    if ((rc = c.add(who, seq, rec_offsets, nullptr, n_records))) return rc;
    return c.finish(who, n_records, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits, stats);
}
