// A database of sketches in one file, and the file entry point of query mode.  Host only.
//   kspider_pack    a directory of .sig / .gz files (kSize > 0) or .bin files (kSize = 0) -> one pack file.  The loaders, and so
//                   the group ids, the names, the k-mer counts and the skipping of a signature without that ksize, are those of
//                   kspider_pairwise_sigs / kspider_pairwise_bins (sketch_loaders.cpp).  The format: sketch_set.h.
//   kspider_query   database and queries, each a pack file or a directory -> the three files of a pairwise run over
//                   database + queries, the TSV holding only the rows of the mode.  The device part is ksp_query_host (query.hip).
//   kspider_gather  database and queries as above -> OUT_kSpider_gather.tsv, the rows of ksp_gather_host (gather.hip).
//   kspider_gather_abund  the same for a directory of query signatures with abundances: the rows of ksp_gather_abund_host, the
//                   weighted columns behind the nine.
//   kspider_compare samples among themselves, or against a database -> OUT_kSpider_compare.tsv (and the matrix), the rows of
//                   ksp_compare_host with the four values of ksp_compare_values, which is here too.
#include <sys/stat.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kspider_amd.h"
#include "engine_internal.h"
#include "index_io.h"
#include "partial_file.h"
#include "sketch_set.h"

namespace {

const char kMagic[8] = {'K', 'S', 'P', 'P', 'A', 'C', 'K', '1'};
constexpr uint32_t kVersion = 1;
constexpr uint64_t kHeaderBytes = 8 + 4 + 4 + 4 * 8;

uint64_t pad8(const uint64_t n) { return (n + 7) & ~7ull; }

template <class T>
void put(std::ofstream& f, const T* p, const uint64_t n, const uint64_t padded_bytes) {
    static const char zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n) f.write((const char*)p, (std::streamsize)(n * sizeof(T)));
    f.write(zeros, (std::streamsize)(padded_bytes - n * sizeof(T)));
}

bool is_directory(const std::string& path) {
    struct stat st;
    return stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

// what a guarded entry throws for a bad argument (KSP_E_ARG instead of KSP_E_IO)
struct ArgError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

template <class Fn>
int guarded(const char* who, Fn fn) {
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const ArgError& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_ARG;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}

// one side of a query: a directory (its kind by kSize) or a pack file, whose kSize must be the caller's when that is not 0
void load_side(const std::string& path, const int kSize, const int threads, ksp::SketchSet& set) {
    if (is_directory(path)) { ksp::sketch_set_from_dir(path, kSize, threads, set); return; }
    ksp::read_sketch_pack(path, set);
    if (kSize != 0 && set.ksize != kSize)
        throw ArgError(path + " was packed with kSize " + std::to_string(set.ksize) + ", not " + std::to_string(kSize));
}

}  // namespace

void ksp::sketch_set_from_dir(const std::string& dir, const int kSize, const int threads, SketchSet& out) {
    SketchNames names;
    std::vector<SketchSource> src;
    if (kSize > 0) load_sig_dir(dir, kSize, threads, names, src);
    else load_bin_dir(dir, threads, names, src);
    SketchSet set;
    set.ksize = kSize;
    const size_t G = names.size();
    set.present.assign(G, 0);
    set.kmers.assign(G, 0);
    set.counted.assign(G, 0);
    bool any_abund = false;
    for (const SketchSource& s : src) any_abund |= s.has_abund;
    for (auto& n : names) set.names.push_back(n.second);   // (ids are 1, 2, ... in this order)
    set.offsets.push_back(0);
    for (const SketchSource& s : src) {   // ascending by id
        set.present[s.id - 1] = 1;
        set.kmers[s.id - 1] = s.kmers;
        set.keys.insert(set.keys.end(), s.run.begin(), s.run.end());
        set.offsets.push_back(set.keys.size());
        set.counted[s.id - 1] = s.has_abund;
        if (any_abund) {
            if (s.has_abund) set.abund.insert(set.abund.end(), s.abund.begin(), s.abund.end());
            else set.abund.resize(set.keys.size(), 0);
        }
    }
    out = std::move(set);
}

void ksp::write_sketch_pack(const std::string& out_path, const SketchSet& set) {
    const uint64_t G = set.names.size(), S = set.offsets.size() - 1, K = set.keys.size();
    std::vector<uint64_t> name_off(G + 1, 0);
    std::string text;
    for (uint64_t g = 0; g < G; ++g) {
        text += set.names[g];
        name_off[g + 1] = text.size();
    }
    const uint64_t B = text.size();
    const uint32_t version = kVersion;
    const int32_t ksize = set.ksize;
    std::ofstream f;
    PartialFiles files;
    files.open(out_path, f);
    f.write(kMagic, 8);
    f.write((const char*)&version, 4);
    f.write((const char*)&ksize, 4);
    for (const uint64_t v : {G, S, K, B}) f.write((const char*)&v, 8);
    put(f, set.kmers.data(), G, pad8(4 * G));
    put(f, set.present.data(), G, pad8(G));
    put(f, set.offsets.data(), S + 1, 8 * (S + 1));
    f.write((const char*)&G, 8);
    put(f, name_off.data(), G + 1, 8 * (G + 1));
    put(f, text.data(), B, pad8(B));
    put(f, set.keys.data(), K, 8 * K);
    files.commit();
}

void ksp::read_sketch_pack(const std::string& path, SketchSet& out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    f.seekg(0, std::ios::end);
    const uint64_t size = (uint64_t)f.tellg();
    f.seekg(0);
    const auto bad = [&](const std::string& what) { return std::runtime_error(path + ": " + what); };
    char head[kHeaderBytes];
    if (size < kHeaderBytes || !f.read(head, kHeaderBytes)) throw bad("shorter than a pack file's header");
    if (std::memcmp(head, kMagic, 8) != 0) throw bad("not a pack file (wrong magic)");
    uint32_t version;
    int32_t ksize;
    uint64_t G, S, K, B;
    std::memcpy(&version, head + 8, 4);
    std::memcpy(&ksize, head + 12, 4);
    std::memcpy(&G, head + 16, 8);
    std::memcpy(&S, head + 24, 8);
    std::memcpy(&K, head + 32, 8);
    std::memcpy(&B, head + 40, 8);
    if (version != kVersion) throw bad("pack version " + std::to_string(version) + ", this reader knows " + std::to_string(kVersion));
    // every count is below the file's size before anything is multiplied or allocated
    if (G > size || S > size || K > size || B > size || S > G) throw bad("counts in the header exceed the file");
    const uint64_t want = kHeaderBytes + pad8(4 * G) + pad8(G) + 8 * (S + 1) + 8 + 8 * (G + 1) + pad8(B) + 8 * K;
    if (size != want) throw bad("is " + std::to_string(size) + " bytes, its header implies " + std::to_string(want));
    SketchSet set;
    set.ksize = ksize;
    std::vector<char> skip(8);
    const auto get = [&](void* p, const uint64_t bytes, const uint64_t padded) {
        if (bytes) f.read((char*)p, (std::streamsize)bytes);
        if (padded > bytes) f.read(skip.data(), (std::streamsize)(padded - bytes));
        if (!f) throw bad("read error");
    };
    set.kmers.resize(G);
    set.present.resize(G);
    set.offsets.resize(S + 1);
    get(set.kmers.data(), 4 * G, pad8(4 * G));
    get(set.present.data(), G, pad8(G));
    get(set.offsets.data(), 8 * (S + 1), 8 * (S + 1));
    uint64_t n_present = 0;
    for (const uint8_t p : set.present) {
        if (p > 1) throw bad("a presence byte is not 0 or 1");
        n_present += p;
    }
    if (n_present != S) throw bad(std::to_string(n_present) + " groups are marked as having a sketch, the header says " + std::to_string(S));
    if (set.offsets[0] != 0) throw bad("the offsets do not start at 0");
    for (uint64_t s = 0; s < S; ++s)
        if (set.offsets[s + 1] < set.offsets[s]) throw bad("the offsets decrease at source " + std::to_string(s));
    if (set.offsets[S] != K) throw bad("the offsets end at " + std::to_string(set.offsets[S]) + ", the header has " + std::to_string(K) + " keys");
    uint64_t name_count = 0;
    get(&name_count, 8, 8);
    if (name_count != G) throw bad("the name count " + std::to_string(name_count) + " disagrees with the header's " + std::to_string(G));
    std::vector<uint64_t> name_off(G + 1);
    std::string text(B, '\0');
    get(name_off.data(), 8 * (G + 1), 8 * (G + 1));
    get(&text[0], B, pad8(B));
    if (name_off[0] != 0) throw bad("the name offsets do not start at 0");
    for (uint64_t g = 0; g < G; ++g)
        if (name_off[g + 1] < name_off[g] || name_off[g + 1] > B) throw bad("the name offsets decrease or leave the text at name " + std::to_string(g));
    if (name_off[G] != B) throw bad("the name offsets do not end at the text's end");
    for (uint64_t g = 0; g < G; ++g) set.names.emplace_back(text, name_off[g], name_off[g + 1] - name_off[g]);
    set.keys.resize(K);
    get(set.keys.data(), 8 * K, 8 * K);
    for (uint64_t s = 0; s < S; ++s)
        for (uint64_t i = set.offsets[s] + 1; i < set.offsets[s + 1]; ++i)
            if (set.keys[i] <= set.keys[i - 1]) throw bad("the run of source " + std::to_string(s) + " is not strictly ascending");
    out = std::move(set);
}

extern "C" int kspider_pack(const char* dir, int kSize, const char* out_path, int user_threads) {
    const char* who = "kspider_pack";
    if (!dir || !out_path || !*out_path) { ksp::set_error(std::string(who) + ": dir or out_path is NULL or empty"); return KSP_E_ARG; }
    if (kSize < 0) { ksp::set_error(std::string(who) + ": kSize is the signatures' ksize, or 0 for .bin sketches"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        ksp::SketchSet set;
        ksp::sketch_set_from_dir(dir, kSize, user_threads, set);
        ksp::write_sketch_pack(out_path, set);
        return (int)KSP_OK;
    });
}

extern "C" int ksp_pack_info(const char* path, uint64_t out[5]) {
    const char* who = "ksp_pack_info";
    if (!path || !out) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        ksp::SketchSet set;
        ksp::read_sketch_pack(path, set);
        uint64_t text = 0;
        for (const std::string& n : set.names) text += n.size();
        out[0] = (uint64_t)(int64_t)set.ksize;
        out[1] = set.names.size();
        out[2] = set.offsets.size() - 1;
        out[3] = set.keys.size();
        out[4] = text;
        return (int)KSP_OK;
    });
}

extern "C" int ksp_pack_load(const char* path, uint32_t* kmers, uint8_t* present, uint64_t* offsets, uint64_t* keys, uint64_t* name_offsets, char* names) {
    const char* who = "ksp_pack_load";
    if (!path || !kmers || !present || !offsets || !keys || !name_offsets || !names) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        ksp::SketchSet set;
        ksp::read_sketch_pack(path, set);
        const size_t G = set.names.size();
        if (G) std::memcpy(kmers, set.kmers.data(), 4 * G);
        if (G) std::memcpy(present, set.present.data(), G);
        std::memcpy(offsets, set.offsets.data(), 8 * set.offsets.size());
        if (!set.keys.empty()) std::memcpy(keys, set.keys.data(), 8 * set.keys.size());
        uint64_t at = 0;
        for (size_t g = 0; g < G; ++g) {
            name_offsets[g] = at;
            std::memcpy(names + at, set.names[g].data(), set.names[g].size());
            at += set.names[g].size();
        }
        name_offsets[G] = at;
        return (int)KSP_OK;
    });
}

extern "C" int kspider_query(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, int mode) {
    const char* who = "kspider_query";
    if (!db || !queries || !out_prefix || !*out_prefix) { ksp::set_error(std::string(who) + ": db, queries and out_prefix are required"); return KSP_E_ARG; }
    if (kSize < 0) { ksp::set_error(std::string(who) + ": kSize is the signatures' ksize, or 0 for .bin sketches"); return KSP_E_ARG; }
    if (mode != KSP_QUERY_CROSS && mode != KSP_QUERY_CROSS_AND_SELF) {
        ksp::set_error(std::string(who) + ": mode is KSP_QUERY_CROSS (0) or KSP_QUERY_CROSS_AND_SELF (1)");
        return KSP_E_ARG;
    }
    return guarded(who, [&]() {
        const int threads = user_threads < 1 ? 1 : user_threads;
        const std::string prefix = out_prefix;
        ksp::SketchSet side[2];
        load_side(db, kSize, threads, side[0]);
        load_side(queries, kSize, threads, side[1]);
        const uint64_t G0 = side[0].names.size(), G = G0 + side[1].names.size();
        if (G > 0xFFFFFFFEull) throw std::runtime_error("more than 2^32 - 2 groups");
        // the sources of both sides by their ids in the union: database 1 .. N, queries N + 1 .. N + Q
        std::vector<uint32_t> id_of[2];
        ksp::IndexData ix;
        std::unordered_map<uint32_t, uint32_t> kmer_count;
        for (int s = 0; s < 2; ++s)
            for (uint64_t g = 0; g < side[s].names.size(); ++g) {
                if (!side[s].present[g]) continue;
                const uint32_t id = (uint32_t)((s ? G0 : 0) + g + 1);
                id_of[s].push_back(id);
                ix.kmer_slots.emplace_back(id, side[s].kmers[g]);
                kmer_count[id] = side[s].kmers[g];
            }
        if (id_of[0].empty() || id_of[1].empty()) throw ArgError(id_of[0].empty() ? "the database has no sketch" : "there is no query sketch");
        ksp_edge* edges = nullptr;
        uint64_t n_edges = 0;
        ksp_query_stats st;
        const char* dv = std::getenv("KSPIDER_DEVICE");
        const int rc = ksp_query_host(side[0].keys.data(), side[0].offsets.data(), (uint32_t)id_of[0].size(), side[1].keys.data(), side[1].offsets.data(),
                                      (uint32_t)id_of[1].size(), mode, dv ? std::atoi(dv) : 0, &edges, &n_edges, &st);
        if (rc != KSP_OK) return rc;
        std::vector<ksp::EdgeRow> rows;
        rows.reserve(n_edges);
        const uint32_t n_db = (uint32_t)id_of[0].size();
        for (uint64_t i = 0; i < n_edges; ++i) {   // ids ascend with the source numbers, so the rows stay sorted
            const ksp_edge& e = edges[i];
            rows.push_back(ksp::EdgeRow{e.source_1 < n_db ? id_of[0][e.source_1] : id_of[1][e.source_1 - n_db], id_of[1][e.source_2 - n_db], e.shared});
        }
        ksp_free(edges);
        // the files only now: a refused or failed query leaves none
        {
            std::ofstream f;
            ksp::PartialFiles files;
            files.open(prefix + ".namesMap", f);
            f << G << "\n";
            for (int s = 0; s < 2; ++s)
                for (uint64_t g = 0; g < side[s].names.size(); ++g) f << (s ? G0 : 0) + g + 1 << " " << side[s].names[g] << "\n";
            files.commit();
        }
        ksp::write_seq_to_kmers(prefix, ix);
        ksp::write_pairwise_tsv(prefix, rows, kmer_count, threads);
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: query: " << st.n_q << " queries against " << st.n_db << " database sources, " << st.passes << " passes, " << n_edges
                      << " rows; table " << st.ms_table << " ms, probe " << st.ms_probe << " ms" << std::endl;
        return (int)KSP_OK;
    });
}

namespace {

// kspider_gather and, weighted, kspider_gather_abund
int gather_files(const char* who, const bool weighted, const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, uint32_t min_hashes,
                 uint32_t max_matches) {
    if (!db || !queries || !out_prefix || !*out_prefix) { ksp::set_error(std::string(who) + ": db, queries and out_prefix are required"); return KSP_E_ARG; }
    if (kSize < 0) { ksp::set_error(std::string(who) + ": kSize is the signatures' ksize, or 0 for .bin sketches"); return KSP_E_ARG; }
    if (min_hashes == 0) { ksp::set_error(std::string(who) + ": min_hashes is 1 or more"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        const int threads = user_threads < 1 ? 1 : user_threads;
        ksp::SketchSet side[2];
        if (weighted && (kSize == 0 || !is_directory(queries))) throw ArgError(std::string(queries) + " is not a directory of signatures (abundances are read from .sig files only)");
        load_side(db, kSize, threads, side[0]);
        load_side(queries, kSize, threads, side[1]);
        if (weighted)
            for (uint64_t g = 0; g < side[1].names.size(); ++g)
                if (side[1].present[g] && !side[1].counted[g]) throw ArgError("the signature of " + side[1].names[g] + " in " + queries + " has no abundances");
        // source s of a side is its s-th group that has a sketch
        std::vector<uint64_t> group_of[2];
        for (int s = 0; s < 2; ++s)
            for (uint64_t g = 0; g < side[s].names.size(); ++g)
                if (side[s].present[g]) group_of[s].push_back(g);
        if (group_of[0].empty() || group_of[1].empty()) throw ArgError(group_of[0].empty() ? "the database has no sketch" : "there is no query sketch");
        if (group_of[0].size() + group_of[1].size() > 0xFFFFFFFEull) throw std::runtime_error("more than 2^32 - 2 groups");
        ksp_gather_row* rows = nullptr;
        ksp_gather_wrow* wrows = nullptr;
        uint64_t n_rows = 0;
        ksp_gather_stats st;
        const char* dv = std::getenv("KSPIDER_DEVICE");
        if (weighted && side[1].abund.size() != side[1].keys.size()) throw std::runtime_error("the queries' abundances are not parallel to their hashes");
        const int rc = weighted ? ksp_gather_abund_host(side[0].keys.data(), side[0].offsets.data(), (uint32_t)group_of[0].size(), side[1].keys.data(), side[1].abund.data(),
                                                        side[1].offsets.data(), (uint32_t)group_of[1].size(), min_hashes, max_matches, dv ? std::atoi(dv) : 0, &wrows, &n_rows, &st)
                                : ksp_gather_host(side[0].keys.data(), side[0].offsets.data(), (uint32_t)group_of[0].size(), side[1].keys.data(), side[1].offsets.data(),
                                                  (uint32_t)group_of[1].size(), min_hashes, max_matches, dv ? std::atoi(dv) : 0, &rows, &n_rows, &st);
        if (rc != KSP_OK) return rc;
        // W of every query
        std::vector<uint64_t> total_w;
        if (weighted)
            for (size_t q = 0; q + 1 < side[1].offsets.size(); ++q) {
                uint64_t w = 0;
                for (uint64_t e = side[1].offsets[q]; e < side[1].offsets[q + 1]; ++e) w += side[1].abund[e];
                total_w.push_back(w);
            }
        // the file only now: a refused or failed call leaves none
        std::string text = "query\trank\tmatch\toverlap\tunique\tf_orig_query\tf_unique_to_query\tf_match\tremaining";
        if (weighted) text += "\tf_unique_weighted\taverage_abund\tmedian_abund\tstd_abund\tn_unique_weighted_found\tsum_weighted_found\ttotal_weighted_hashes";
        text += "\n";
        char buf[32];
        for (uint64_t i = 0; i < n_rows; ++i) {
            const ksp_gather_wrow* w = weighted ? &wrows[i] : nullptr;
            const ksp_gather_row r = w ? ksp_gather_row{w->query, w->rank, w->source, w->overlap, w->unique, w->remaining} : rows[i];
            const float q_size = (float)(side[1].offsets[r.query + 1] - side[1].offsets[r.query]), s_size = (float)(side[0].offsets[r.source + 1] - side[0].offsets[r.source]);
            text += side[1].names[group_of[1][r.query]] + "\t" + std::to_string(r.rank) + "\t" + side[0].names[group_of[0][r.source]] + "\t" + std::to_string(r.overlap) + "\t" +
                    std::to_string(r.unique);
            for (const float v : {(float)r.overlap / q_size, (float)r.unique / q_size, (float)r.overlap / s_size}) {
                text += "\t";
                text.append(buf, (size_t)ksp::format_float(buf, v));
            }
            text += "\t" + std::to_string(r.remaining);
            if (w) {
                typedef unsigned __int128 u128;
                const uint64_t W = total_w[r.query];
                const u128 sq = ((u128)w->sq_hi << 64) | w->sq_lo, mean2 = (u128)w->w_unique * w->w_unique;
                const u128 spread = (u128)r.unique * sq - mean2;   // n Σa² - (Σa)² >= 0: exact, rounded once below
                for (const float v : {W ? (float)((double)w->w_unique / (double)W) : 0.0f /* a query of abundances 0 */,(float)((double)w->w_unique / (double)r.unique), (float)((double)w->median2 / 2.0),
                                      (float)(std::sqrt((double)spread) / (double)r.unique)}) {
                    text += "\t";
                    text.append(buf, (size_t)ksp::format_float(buf, v));
                }
                text += "\t" + std::to_string(w->w_unique) + "\t" + std::to_string(w->w_found) + "\t" + std::to_string(W);
            }
            text += "\n";
        }
        ksp_free(rows);
        ksp_free(wrows);
        {
            std::ofstream f;
            ksp::PartialFiles files;
            files.open(std::string(out_prefix) + "_kSpider_gather.tsv", f);
            f.write(text.data(), (std::streamsize)text.size());
            files.commit();
        }
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: gather: " << st.n_q << " queries against " << st.n_db << " database sources, " << st.passes << " passes, " << st.candidates
                      << " candidates, " << st.rounds << " rounds (" << st.tail_rounds << " in the tail), " << n_rows << " rows; table " << st.ms_table << " ms, candidates "
                      << st.ms_candidates << " ms, fill " << st.ms_fill << " ms, rounds " << st.ms_rounds << " ms" << std::endl;
        return (int)KSP_OK;
    });
}

}  // namespace

extern "C" int kspider_gather(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, uint32_t min_hashes, uint32_t max_matches) {
    return gather_files("kspider_gather", false, db, queries, kSize, out_prefix, user_threads, min_hashes, max_matches);
}

extern "C" int kspider_gather_abund(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, uint32_t min_hashes, uint32_t max_matches) {
    return gather_files("kspider_gather_abund", true, db, queries, kSize, out_prefix, user_threads, min_hashes, max_matches);
}

extern "C" int ksp_compare_values(const ksp_wedge* row, uint64_t /*n_1*/, uint64_t sum_1, uint64_t sumsq_1, uint64_t /*n_2*/, uint64_t sum_2, uint64_t sumsq_2, double out[4]) {
    if (!row || !out) { ksp::set_error("ksp_compare_values: NULL argument"); return KSP_E_ARG; }
    if (!sum_1 || !sumsq_1 || !sum_2 || !sumsq_2) { ksp::set_error("ksp_compare_values: a source's total is 0"); return KSP_E_ARG; }
    typedef unsigned __int128 u128;
    const bool same = (u128)row->dot * row->dot == (u128)sumsq_1 * sumsq_2;   // the vectors are parallel: exactly 1, whatever the roots round to
    const double cosine = same ? 1.0 : std::min(1.0, (double)row->dot / (std::sqrt((double)sumsq_1) * std::sqrt((double)sumsq_2)));
    out[0] = cosine;
    out[1] = 1.0 - 2.0 * std::acos(cosine) / 3.14159265358979323846;
    out[2] = (double)row->mass_1 / (double)sum_1;
    out[3] = (double)row->mass_2 / (double)sum_2;
    return KSP_OK;
}

namespace {

// The sources of a loaded side as ksp_compare_host takes them: source s is the side's s-th group that has a sketch (group_of[s]),
// and abund is empty for a side without any counted sketch, else parallel to the keys with 1 for every hash of a flat sketch.
struct CompareSide {
    ksp::SketchSet set;
    std::vector<uint64_t> group_of;
    std::vector<uint32_t> abund;
    void load(const std::string& path, const int kSize, const int threads) {
        load_side(path, kSize, threads, set);
        for (uint64_t g = 0; g < set.names.size(); ++g)
            if (set.present[g]) group_of.push_back(g);
        if (set.abund.empty()) return;
        if (set.abund.size() != set.keys.size()) throw std::runtime_error("the abundances of " + path + " are not parallel to their hashes");
        abund = set.abund;
        for (size_t s = 0; s < group_of.size(); ++s)
            if (!set.counted[group_of[s]]) std::fill(abund.begin() + (std::ptrdiff_t)set.offsets[s], abund.begin() + (std::ptrdiff_t)set.offsets[s + 1], 1u);
    }
    uint32_t n() const { return (uint32_t)group_of.size(); }
};

}  // namespace

extern "C" int kspider_compare(const char* samples, const char* against, int kSize, const char* out_prefix, int user_threads, uint64_t flags) {
    const char* who = "kspider_compare";
    if (!samples || !out_prefix || !*out_prefix) { ksp::set_error(std::string(who) + ": samples and out_prefix are required"); return KSP_E_ARG; }
    if (kSize < 0) { ksp::set_error(std::string(who) + ": kSize is the signatures' ksize, or 0 for .bin sketches"); return KSP_E_ARG; }
    if (flags & ~KSP_COMPARE_MATRIX) { ksp::set_error(std::string(who) + ": unknown flags"); return KSP_E_ARG; }
    const bool matrix = (flags & KSP_COMPARE_MATRIX) != 0;
    if (matrix && against) { ksp::set_error(std::string(who) + ": the matrix is of the samples among themselves, not of samples against a database"); return KSP_E_ARG; }
    return guarded(who, [&]() {
        const int threads = user_threads < 1 ? 1 : user_threads;
        const std::string prefix = out_prefix;
        CompareSide side[2];   // [0] the database (empty without `against`), [1] the samples
        if (against) side[0].load(against, kSize, threads);
        side[1].load(samples, kSize, threads);
        const uint64_t G0 = side[0].set.names.size(), G1 = side[1].set.names.size(), G = G0 + G1;
        if (G > 0xFFFFFFFEull) throw std::runtime_error("more than 2^32 - 2 groups");
        if (against && side[0].n() == 0) throw ArgError("the database has no sketch");
        if (side[1].n() == 0) throw ArgError("there is no sample sketch");
        if (matrix && G1 > KSP_COMPARE_MATRIX_MAX) {
            ksp::set_error(std::string(who) + ": a matrix of " + std::to_string(G1) + " samples (the limit is " + std::to_string(KSP_COMPARE_MATRIX_MAX) + ")");
            return (int)KSP_E_LIMIT;
        }
        const uint32_t n_db = side[0].n(), n_q = side[1].n();
        ksp_wedge* rows = nullptr;
        uint64_t n_rows = 0;
        ksp_compare_stats st;
        std::vector<uint64_t> sum((size_t)n_db + n_q), sumsq((size_t)n_db + n_q);
        const char* dv = std::getenv("KSPIDER_DEVICE");
        const int rc = ksp_compare_host(n_db ? side[0].set.keys.data() : nullptr, side[0].abund.empty() ? nullptr : side[0].abund.data(), n_db ? side[0].set.offsets.data() : nullptr, n_db,
                                        side[1].set.keys.data(), side[1].abund.empty() ? nullptr : side[1].abund.data(), side[1].set.offsets.data(), n_q,
                                        against ? KSP_QUERY_CROSS : KSP_QUERY_CROSS_AND_SELF, dv ? std::atoi(dv) : 0, &rows, &n_rows, sum.data(), sumsq.data(), &st);
        if (rc != KSP_OK) return rc;
        // source s of the call -> its side, its index there, its id in the union: database 1 .. N, samples N + 1 .. N + Q
        const auto id_of = [&](const uint32_t s) { return (uint32_t)(s < n_db ? side[0].group_of[s] + 1 : G0 + side[1].group_of[s - n_db] + 1); };
        const auto keys_of = [&](const uint32_t s) {
            const std::vector<uint64_t>& off = s < n_db ? side[0].set.offsets : side[1].set.offsets;
            const uint32_t i = s < n_db ? s : s - n_db;
            return off[i + 1] - off[i];
        };
        std::string text = "source_1\tsource_2\tshared_kmers\tdot\tmass_1\tmass_2\tcosine\tangular_similarity\tweighted_containment_1\tweighted_containment_2\n";
        std::vector<float> cells;   // the matrix, by group of the samples
        if (matrix) {
            cells.assign((size_t)G1 * G1, 0.0f);
            for (uint64_t g = 0; g < G1; ++g) cells[(size_t)(g * G1 + g)] = 1.0f;
        }
        char buf[256];
        for (uint64_t i = 0; i < n_rows; ++i) {   // ids ascend with the source numbers, so the rows stay sorted
            const ksp_wedge& r = rows[i];
            double v[4];
            if (ksp_compare_values(&r, keys_of(r.source_1), sum[r.source_1], sumsq[r.source_1], keys_of(r.source_2), sum[r.source_2], sumsq[r.source_2], v) != KSP_OK) {
                ksp_free(rows);
                throw std::runtime_error("a row names a source without abundance");
            }
            char angular[32];
            std::snprintf(angular, sizeof angular, "%.6g", v[1]);
            const int n = std::snprintf(buf, sizeof buf, "%u\t%u\t%llu\t%llu\t%llu\t%llu\t%.6g\t%s\t%.6g\t%.6g\n", id_of(r.source_1), id_of(r.source_2), (unsigned long long)r.shared,
                                        (unsigned long long)r.dot, (unsigned long long)r.mass_1, (unsigned long long)r.mass_2, v[0], angular, v[2], v[3]);
            text.append(buf, (size_t)n);
            if (matrix) {   // six significant digits survive a float, so "%.6g" of the cell is the TSV's text again
                const uint64_t a = side[1].group_of[r.source_1], b = side[1].group_of[r.source_2];
                cells[(size_t)(a * G1 + b)] = cells[(size_t)(b * G1 + a)] = std::strtof(angular, nullptr);
            }
        }
        ksp_free(rows);
        // the files only now: a refused or failed call leaves none
        ksp::IndexData ix;
        for (int s = 0; s < 2; ++s)
            for (const uint64_t g : side[s].group_of) ix.kmer_slots.emplace_back((uint32_t)((s ? G0 : 0) + g + 1), side[s].set.kmers[g]);
        {
            std::ofstream f;
            ksp::PartialFiles files;
            files.open(prefix + ".namesMap", f);
            f << G << "\n";
            for (int s = 0; s < 2; ++s)
                for (uint64_t g = 0; g < side[s].set.names.size(); ++g) f << (s ? G0 : 0) + g + 1 << " " << side[s].set.names[g] << "\n";
            files.commit();
        }
        ksp::write_seq_to_kmers(prefix, ix);
        ksp::write_file_atomically(prefix + "_kSpider_compare.tsv", text);
        if (matrix) {
            std::string csv;
            for (uint64_t g = 0; g < G1; ++g) csv += (g ? "," : "") + side[1].set.names[g];
            csv += "\n";
            for (uint64_t a = 0; a < G1; ++a) {
                for (uint64_t b = 0; b < G1; ++b) {
                    const int n = std::snprintf(buf, sizeof buf, "%s%.6g", b ? "," : "", (double)cells[(size_t)(a * G1 + b)]);
                    csv.append(buf, (size_t)n);
                }
                csv += "\n";
            }
            ksp::write_file_atomically(prefix + "_kSpider_compare_matrix.csv", csv);
        }
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: compare: " << st.n_q << " samples" << (against ? " against " + std::to_string(st.n_db) + " database sources" : std::string()) << ", "
                      << st.passes << " passes, " << n_rows << " rows; totals " << st.ms_totals << " ms, table " << st.ms_table << " ms, holders " << st.ms_holders
                      << " ms, probe " << st.ms_probe << " ms" << std::endl;
        return (int)KSP_OK;
    });
}
