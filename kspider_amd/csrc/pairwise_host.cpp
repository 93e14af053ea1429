// kSpider::pairwise() drop-in: host side.
//
// Mirrors /root/reference/src/pairwise.cpp:123-276 phase by phase:
//   :127-129  load colour -> sources            -> ksp::load_index
//   :136-137  load colour counts                -> ksp::load_index
//   :166-181  load k-mer counts, write seqToKmersNo.tsv
//   :194-237  accumulate shared k-mers per pair -> MI355X engine (engine.hip)
//   :242-275  write pairwise.tsv (float maths + formatting on the host)
// kspider_pairwise_ani[_and_cluster] add the ANI column of `pairwise --estimate-ani` (ks_pairwise.py:29-84, ani.h).
// The same progress lines go to stdout.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kSpider.hpp"
#include "../../include/kspider_amd.h"
#include "ani.h"
#include "engine_internal.h"
#include "index_io.h"

namespace ksp {
std::vector<int> devices_from_env() {
    std::vector<int> out;
    if (const char* ds = std::getenv("KSPIDER_DEVICES")) {
        const char* p = ds;
        while (*p) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) break;
            out.push_back((int)v);
            p = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') break;
        }
    }
    if (out.empty()) {
        int device = 0;
        if (const char* d = std::getenv("KSPIDER_DEVICE")) device = std::atoi(d);
        out.push_back(device);
    }
    return out;
}
}  // namespace ksp

// a kept row names its nodes by id - 1: the ids must be rows of .namesMap
void ksp::check_row_nodes(const long long a, const long long b, const uint64_t N) {
    if (a < 1 || b < 1 || (uint64_t)a > N || (uint64_t)b > N)
        throw std::runtime_error("pairwise row names node " + std::to_string(std::max(a, b)) + " but .namesMap has " + std::to_string(N) + " rows (ids must be 1..N)");
}

namespace {

typedef std::chrono::high_resolution_clock Clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
using ksp::AfterJoin;

// One drop-in call.  after.kind: what is also taken from the edges while they are on the device —
//   kCluster  the cluster file of `kSpider cluster` (ks_clustering.py:63-137); col 6 clusters on the ANI column
//   kRepr     the ranking of the sources by their neighbour counts (apps/repr_sketches.cpp:27-33,38-43)
//   kCut      only the rows that pass a containment cut are wanted: the edges are cut on the device, directly after the join
//   kSweep    the cluster file at every cut-off of a ladder, from one pass over the edges
//   kTree     the single-linkage tree: the maximum spanning forest of the edges
//   kDerep    the dereplicated set: greedy representatives in rank order and the members they stand for
//   kTopk     the k best hits of every source
//   kReport   the report of every cluster at one cut-off: density, value range, medoid, coverage, and the members' table
//   kUpgma    the average-linkage tree: the exact UPGMA merges of the edges
struct PairwiseJob {
    std::string prefix;
    int threads = 1;
    bool ani = false;       // also write the ANI column of `pairwise --estimate-ani` (ks_pairwise.py:29-84; k from PREFIX.extra)
    AfterJoin after;
    std::string dist;       // kSweep, kTree, kReport, kUpgma: the distance's name in their file names
    std::string repr_out;   // kRepr: "" = PREFIX_kSpider_repr_sketches.txt; kDerep: "" = PREFIX_kSpider_dereplicated_<dist>.tsv;
                            // kTopk: "" = PREFIX_kSpider_topk_<dist>.tsv
    bool newick = false;    // kTree, kUpgma
    PairwiseJob(const char* index_prefix, int user_threads, AfterJoin::Kind kind = AfterJoin::kNone, int col = 0)
        : prefix(index_prefix), threads(user_threads < 1 ? 1 : user_threads) { after.kind = kind; after.col = col; }
};

// the colour index as the engine takes it: an inverted index over dense source indices
struct Postings {
    std::vector<uint32_t> ids;        // group id of every source index, ascending
    std::vector<uint32_t> dense_of;   // direct table id -> index when the id space is small enough
    std::vector<uint64_t> key_off;
    std::vector<uint32_t> post_src, key_w;
    std::vector<std::pair<uint32_t, uint32_t>> zero_pairs;   // pairs of ids touched through weight-0 colours: sorted, each once
    std::vector<uint32_t> counts;     // k-mer count of every source index (only where something after the join reads them)
    uint32_t dense(uint32_t g) const {
        return dense_of.empty() ? (uint32_t)(std::lower_bound(ids.begin(), ids.end(), g) - ids.begin()) : dense_of[g];
    }
};
// a row that exists only with shared_kmers = 0 (the pair shares colours of weight 0 and no other), by its source indices
struct ZeroRow { uint32_t a, b; };
struct ForestEdge { uint32_t a, b; float v; };   // source indices and the column's value
// kTopk: per source index the number of its hits; the other end (a source index) and the column's value of every hit, flat in source order
struct TopkHits { std::vector<uint32_t> count, neighbour; std::vector<float> value; };

// column 3 / 4 / 5 of a row as the TSV writer computes it (index_io.cpp format_rows = src/pairwise.cpp:260-264; beside
// ksp::row_min_max, whose min + max is not c12 + c21 when one of them is a NaN)
float column_value(const int col, const uint64_t shared, const uint32_t n1, const uint32_t n2) {
    const float c12 = (float)shared / n2, c21 = (float)shared / n1;
    return col == 3 ? std::min(c12, c21) : col == 5 ? std::max(c12, c21) : (float)((double)(c12 + c21) / 2.0);
}
// the reference's threshold test on the float, by ksp::cc_critical's vcrit / mode (mode 1: only NaN rows pass)
bool passes_cut(const float v, const float vcrit, const int mode) { return mode ? v != v : !(v < vcrit); }

// union-find over parent[] (parent[v] == v: a root): the larger root goes under the smaller
uint32_t find_root(uint32_t* parent, uint32_t v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
}
bool unite(uint32_t* parent, const uint32_t a, const uint32_t b) {   // false: they were united already
    const uint32_t ra = find_root(parent, a), rb = find_root(parent, b);
    if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    return ra != rb;
}
// the rows z with keeps(z) united into lab (per source index the smallest index of its component); returns how many it kept
template <class Keeps>
uint64_t unite_rows(uint32_t* lab, const uint32_t N, const std::vector<ZeroRow>& rows, Keeps&& keeps) {
    uint64_t n_kept = 0;
    bool merged = false;
    for (size_t z = 0; z < rows.size(); ++z) {
        if (!keeps(z)) continue;
        ++n_kept;
        if (unite(lab, rows[z].a, rows[z].b)) merged = true;
    }
    if (merged) for (uint32_t s = 0; s < N; ++s) lab[s] = find_root(lab, s);
    return n_kept;
}
// labels per source index -> labels per .namesMap node (id - 1), NN of them
void node_labels_of(const std::vector<uint32_t>& ids, const uint32_t* lab, const uint64_t NN, uint32_t* node_label) {
    for (uint64_t v = 0; v < NN; ++v) node_label[v] = (uint32_t)v;
    for (uint32_t i = 0; i < (uint32_t)ids.size(); ++i) {
        if (lab[i] == i) continue;   // (a root, or a source without a kept edge)
        ksp::check_row_nodes(ids[i], ids[lab[i]], NN);
        node_label[ids[i] - 1] = ids[lab[i]] - 1;
    }
}

// src/pairwise.cpp:127-155: the index and what is refused about it before any file is written, with the reference's progress line
int load_inputs(const PairwiseJob& job, ksp::IndexData& ix, std::vector<std::string>& derep_names) {
    auto t0 = Clock::now();
    ksp::load_index(job.prefix, ix);
    if (job.after.kind == AfterJoin::kDerep || job.after.kind == AfterJoin::kTopk || job.after.kind == AfterJoin::kReport || job.after.kind == AfterJoin::kUpgma) {   // every source must be a row of .namesMap: refused before any file is written
        ksp::read_names_map(job.prefix, derep_names);
        for (auto& c : ix.colors)
            for (uint32_t g : c.second) ksp::check_row_nodes(g, g, derep_names.size());
    }
    if (job.after.kind == AfterJoin::kRepr)   // the reference tool reads the ids with stoi: refused before any file is written
        for (auto& c : ix.colors)
            for (uint32_t g : c.second)
                if (g > 2147483647u) {
                    ksp::set_error("kspider_pairwise_and_repr: group id " + std::to_string(g) + " exceeds 2^31 - 1 (the reference tool reads ids as int)");
                    return KSP_E_LIMIT;
                }
    std::cout << "mapping colors to groups: " << since(t0) << " secs" << std::endl;
    return KSP_OK;
}
// src/pairwise.cpp:156-181: PREFIX_kSpider_seqToKmersNo.tsv, the first file of a call, and the k-mer counts, with the reference's progress lines
void write_kmer_counts(const PairwiseJob& job, const ksp::IndexData& ix, std::unordered_map<uint32_t, uint32_t>& kmer_count) {
    auto t0 = Clock::now();
    std::cout << "parsing index colors: " << since(t0) << " secs" << std::endl;
    t0 = Clock::now();
    ksp::write_seq_to_kmers(job.prefix, ix);
    for (auto& s : ix.kmer_slots) kmer_count[s.first] = s.second;
    std::cout << "kmer counting: " << since(t0) << " secs" << std::endl;
}

// The colour index IS an inverted index (colour -> sources, src/pairwise.cpp:128-170): hand it to the
// engine as postings — no transposition into per-source runs, no sort and prune on the device.
void index_postings(const ksp::IndexData& ix, Postings& P) {
    // dense source index = rank of the group ID, so that index order == ID order and the
    // engine's (i < j) is the reference's ascending(source_1, source_2) (:73-78, :218)
    uint32_t max_id = 0;
    for (auto& c : ix.colors)
        for (uint32_t g : c.second) max_id = std::max(max_id, g);
    std::vector<uint32_t>& ids = P.ids;
    if (max_id < (1u << 28)) {
        std::vector<uint8_t> seen((size_t)max_id + 1, 0);
        for (auto& c : ix.colors)
            for (uint32_t g : c.second) seen[g] = 1;
        P.dense_of.assign((size_t)max_id + 1, 0);
        for (uint32_t g = 0; g <= max_id; ++g)
            if (seen[g]) { P.dense_of[g] = (uint32_t)ids.size(); ids.push_back(g); }
        if (ix.colors.empty()) ids.clear();
    } else {
        for (auto& c : ix.colors) ids.insert(ids.end(), c.second.begin(), c.second.end());
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    std::vector<uint64_t> wsum(ids.size(), 0);
    P.key_off.push_back(0);
    {
        size_t total = 0;
        for (auto& c : ix.colors) total += c.second.size() >= 2 ? c.second.size() : 0;
        P.post_src.reserve(total);
        P.key_off.reserve(ix.colors.size() + 1);
        P.key_w.reserve(ix.colors.size());
    }
    for (auto& c : ix.colors) {
        uint32_t w = 0;
        if (!ix.colors_count.find(c.first, w)) w = 0;   // colorsCount[item.first] (:221): 0 when absent
        if (c.second.size() < 2) continue;          // a colour with one source produces no pair
        if (w == 0) {
            // the reference still creates the pair entries (with += 0): remember them
            for (size_t x = 0; x < c.second.size(); ++x)
                for (size_t y = x + 1; y < c.second.size(); ++y) {
                    uint32_t a = c.second[x], b = c.second[y];
                    if (a > b) std::swap(a, b);
                    if (a != b) P.zero_pairs.emplace_back(a, b);
                }
            continue;
        }
        for (uint32_t g : c.second) {
            const uint32_t di = P.dense(g);
            P.post_src.push_back(di);
            wsum[di] += w;
        }
        P.key_off.push_back(P.post_src.size());
        P.key_w.push_back(w);
    }
    // (a source cannot repeat inside a colour: flat_hash_set; two colours narrowing to the same uint32 id
    //  were resolved by load_index the way insert_or_assign does)
    for (size_t s = 0; s < ids.size(); ++s)
        if (wsum[s] >= (1ull << 32))
            throw std::runtime_error("kspider_amd: colour weights of group " + std::to_string(ids[s]) +
                                     " sum to >= 2^32 (32-bit pair counters would overflow)");
    std::sort(P.zero_pairs.begin(), P.zero_pairs.end());
    P.zero_pairs.erase(std::unique(P.zero_pairs.begin(), P.zero_pairs.end()), P.zero_pairs.end());
}

// The device's edges and the weight-0 pairs as the rows of the TSV, in its order.  Returns the rows that exist only with
// shared_kmers = 0, in (source_1, source_2) order (kCut: the kept ones, the undecided of them last).
std::vector<ZeroRow> merge_rows(const ksp::IndexData& ix, const Postings& P, const AfterJoin& after, const ksp_edge* edges, const uint64_t n_edges,
                                std::vector<ksp::EdgeRow>& rows) {
    rows.reserve(n_edges + P.zero_pairs.size());
    for (uint64_t i = 0; i < n_edges; ++i)
        rows.push_back(ksp::EdgeRow{P.ids[edges[i].source_1], P.ids[edges[i].source_2], edges[i].shared});
    std::vector<ZeroRow> zero_rows;
    if (P.zero_pairs.empty()) return zero_rows;
    const bool cut = after.kind == AfterJoin::kCut;
    float vcrit = 0;
    int mode = 0;
    if (cut) ksp::cc_critical(after.cutoff, &vcrit, &mode);
    const bool device_drops = mode || vcrit > 0;   // (otherwise every row passes: no value is negative)
    std::vector<std::pair<uint32_t, uint32_t>> unsure;   // kept as a shared-0 row, unless the device dropped a real row of the pair
    for (auto& zp : P.zero_pairs) {
        const uint32_t a = P.dense(zp.first), b = P.dense(zp.second);
        // the cut of such a row: the same test with the same vcrit / mode, on the host
        if (cut && !passes_cut(column_value(after.col, 0, P.counts[a], P.counts[b]), vcrit, mode)) continue;
        auto it = std::lower_bound(rows.begin(), rows.end(), zp, [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
            return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
        });
        if (it != rows.end() && it->source_1 == zp.first && it->source_2 == zp.second) continue;   // (the pair also shares a weighted colour: an ordinary row)
        if (cut && device_drops) unsure.push_back(zp);
        else zero_rows.push_back(ZeroRow{a, b});
    }
    if (!unsure.empty()) {
        // Only a NaN row gets here (a source of 0 k-mers): its pair is not among the kept rows, so either it shares no weighted
        // colour — the shared-0 row is a row of the full TSV, and kept — or the device dropped its real row.  The colours decide.
        std::vector<uint8_t> real(unsure.size(), 0);
        for (auto& c : ix.colors) {
            uint32_t w = 0;
            if (c.second.size() < 2 || !ix.colors_count.find(c.first, w) || w == 0) continue;
            std::vector<uint32_t> members(c.second.begin(), c.second.end());
            std::sort(members.begin(), members.end());
            for (size_t u = 0; u < unsure.size(); ++u)
                if (!real[u] && std::binary_search(members.begin(), members.end(), unsure[u].first) &&
                    std::binary_search(members.begin(), members.end(), unsure[u].second))
                    real[u] = 1;
        }
        for (size_t u = 0; u < unsure.size(); ++u)
            if (!real[u]) zero_rows.push_back(ZeroRow{P.dense(unsure[u].first), P.dense(unsure[u].second)});
    }
    for (auto& z : zero_rows) rows.push_back(ksp::EdgeRow{P.ids[z.a], P.ids[z.b], 0});
    std::sort(rows.begin(), rows.end(), [](const ksp::EdgeRow& a, const ksp::EdgeRow& b) {
        return a.source_1 != b.source_1 ? a.source_1 < b.source_1 : a.source_2 < b.source_2;
    });
    return zero_rows;
}

// a row of a weight-0 colour with a source of 0 k-mers has a NaN containment, so no ANI
int refuse_nan_rows(const std::vector<ksp::EdgeRow>& rows, const std::unordered_map<uint32_t, uint32_t>& kmer_count) {
    for (auto& r : rows) {
        if (r.shared) continue;
        auto i1 = kmer_count.find(r.source_1), i2 = kmer_count.find(r.source_2);
        float mn, mx;
        ksp::row_min_max(0, i1 == kmer_count.end() ? 0 : i1->second, i2 == kmer_count.end() ? 0 : i2->second, &mn, &mx);
        if (mn != mn || mx != mx) {
            ksp::set_error("pairwise row " + std::to_string(r.source_1) + "\t" + std::to_string(r.source_2) +
                           " has a NaN containment (0 shared k-mers of a source with 0 k-mers): it has no ANI");
            return KSP_E_ARG;
        }
    }
    return KSP_OK;
}

// ---- one finisher per kind: what the device found on the join's own edge records, the shared-0 rows (rows of the TSV too, with
// the value 0, or NaN beside a source of 0 k-mers) taken in on the host, and the files ----

void finish_repr(PairwiseJob& job, const Postings& P, const std::vector<ZeroRow>& zero_rows) {
    AfterJoin& A = job.after;
    // a shared-0 row passes a negative threshold only — the same text test, and the ranking redone with their counts
    std::vector<uint32_t> extra;
    for (auto& z : zero_rows)
        if (ksp::repr_text_passes(column_value(A.col, 0, P.counts[z.a], P.counts[z.b]), A.threshold)) {
            extra.push_back(z.a);
            extra.push_back(z.b);
        }
    if (!extra.empty()) {
        std::vector<uint32_t> degree(P.ids.size(), 0);
        for (size_t i = 0; i < A.node.size(); ++i) degree[A.node[i]] = A.count[i];
        for (uint32_t v : extra) ++degree[v];
        A.node.clear();
        for (uint32_t v = 0; v < (uint32_t)P.ids.size(); ++v)
            if (degree[v]) A.node.push_back(v);
        std::stable_sort(A.node.begin(), A.node.end(), [&](uint32_t x, uint32_t y) { return degree[x] > degree[y]; });
        A.count.resize(A.node.size());
        for (size_t i = 0; i < A.node.size(); ++i) A.count[i] = degree[A.node[i]];
    }
    ksp::write_repr_file(job.repr_out.empty() ? job.prefix + "_kSpider_repr_sketches.txt" : job.repr_out, P.ids, A.node.data(), A.count.data(),
                         A.node.size());
    if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: " << A.node.size() << " sources with a neighbour ranked" << std::endl;
}

void finish_cluster(PairwiseJob& job, const Postings& P, const std::vector<ZeroRow>& zero_rows, const uint64_t n_edges, const double* ani_tab) {
    AfterJoin& A = job.after;
    const uint32_t N = (uint32_t)P.ids.size();
    std::vector<std::string> name_of;
    ksp::read_names_map(job.prefix, name_of);
    if (n_edges == 0) for (uint32_t i = 0; i < N; ++i) A.labels[i] = i;   // (no edges at all: the device pass did not run)
    float vcrit = 0;
    int mode = 0;
    ksp::cc_critical(A.cutoff, &vcrit, &mode);
    unite_rows(A.labels.data(), N, zero_rows, [&](const size_t z) {
        const uint32_t n1 = P.counts[zero_rows[z].a], n2 = P.counts[zero_rows[z].b];
        if (A.col != 6) return passes_cut(column_value(A.col, 0, n1, n2), vcrit, mode);
        double g = 0;   // (the NaN rows were refused before the TSV was written)
        ksp::ani_of_row(column_value(3, 0, n1, n2), column_value(5, 0, n1, n2), ani_tab, &g);
        return !(g * 100.0 < A.cutoff * 100.0);
    });
    std::vector<uint32_t> node_label(name_of.size());
    node_labels_of(P.ids, A.labels.data(), name_of.size(), node_label.data());
    ksp::write_cluster_file(job.prefix, A.cutoff * 100.0, node_label, name_of);
    if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: clusters from " << A.n_kept << " edges that pass the cut" << std::endl;
}

void finish_sweep(PairwiseJob& job, const Postings& P, const std::vector<ZeroRow>& zero_rows, const uint64_t n_edges) {
    AfterJoin& A = job.after;
    const uint32_t N = (uint32_t)P.ids.size(), K = A.n_cutoffs;
    std::vector<std::string> name_of;
    ksp::read_names_map(job.prefix, name_of);
    const uint64_t NN = name_of.size();
    std::vector<float> zero_val;
    for (auto& z : zero_rows) zero_val.push_back(column_value(A.col, 0, P.counts[z.a], P.counts[z.b]));
    std::vector<uint32_t> node_labels((size_t)K * NN);
    for (uint32_t i = 0; i < K; ++i) {   // the same test per cut-off, and the row united into every rank it passes
        uint32_t* lab = A.labels.data() + (size_t)i * N;
        float vcrit = 0;
        int mode = 0;
        ksp::cc_critical(A.cutoffs[i], &vcrit, &mode);
        A.kept[i] += unite_rows(lab, N, zero_rows, [&](const size_t z) { return passes_cut(zero_val[z], vcrit, mode); });
        node_labels_of(P.ids, lab, NN, node_labels.data() + (size_t)i * NN);
    }
    ksp::write_sweep_outputs(job.prefix, job.dist, A.cutoffs, K, node_labels.data(), A.kept.data(), name_of);
    if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: clusters at " << K << " cut-offs from one pass over " << n_edges << " edges" << std::endl;
}

// the forest's rows, while the device's records are still here: the value as the writer computes it
std::vector<ForestEdge> device_forest(const AfterJoin& A, const Postings& P, const ksp_edge* edges, const uint64_t n_edges) {
    std::vector<ForestEdge> forest;
    for (const uint32_t e : A.index) {
        if (e >= n_edges) throw std::runtime_error("tree: the device named a record that does not exist");
        forest.push_back(ForestEdge{edges[e].source_1, edges[e].source_2,
                                    column_value(A.col, edges[e].shared, P.counts[edges[e].source_1], P.counts[edges[e].source_2])});
    }
    return forest;
}

void finish_tree(PairwiseJob& job, const Postings& P, const std::vector<ZeroRow>& zero_rows, const uint64_t n_edges, std::vector<ForestEdge>& forest) {
    const uint32_t N = (uint32_t)P.ids.size();
    std::vector<std::string> name_of;
    ksp::read_names_map(job.prefix, name_of);
    // the shared-0 rows are united in after the device's forest, in (source_1, source_2) order
    const size_t n_device = forest.size();
    for (auto& z : zero_rows) forest.push_back(ForestEdge{z.a, z.b, column_value(job.after.col, 0, P.counts[z.a], P.counts[z.b])});
    // Kruskal over (the device's forest) + (the shared-0 rows): an edge the device left out closes a cycle of better edges in
    // its graph, so it does in the larger one.  Order: NaN first, then the float descending, then the device's merge order,
    // then the shared-0 rows in (source_1, source_2) order — a stable sort of what is already in that order.
    std::vector<uint32_t> order(forest.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (uint32_t)i;
    if (forest.size() > n_device)
        std::stable_sort(order.begin(), order.end(), [&](const uint32_t x, const uint32_t y) {
            const float vx = forest[x].v, vy = forest[y].v;
            const bool nx = vx != vx, ny = vy != vy;
            if (nx || ny) return nx && !ny;
            return vx > vy;
        });
    std::vector<uint32_t> parent((size_t)N);
    for (uint32_t i = 0; i < N; ++i) parent[i] = i;
    std::vector<ksp::TreeRow> tree_rows;
    for (const uint32_t i : order) {
        const ForestEdge& fe = forest[i];
        if (!unite(parent.data(), fe.a, fe.b)) continue;
        const uint32_t a = P.ids[fe.a], b = P.ids[fe.b];
        ksp::check_row_nodes(a, b, name_of.size());
        char buf[64];
        buf[ksp::format_float(buf, fe.v)] = 0;
        const double d = std::strtod(buf, nullptr);
        tree_rows.push_back(ksp::TreeRow{a - 1, b - 1, d * 100.0, d, buf});
    }
    ksp::write_tree_files(job.prefix, job.dist, tree_rows, name_of, job.newick);
    if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: tree of " << tree_rows.size() << " merges from " << n_edges << " edges" << std::endl;
}

// the value text of every member's assigning record, while the device's records are still here: the writer's float, its text
std::vector<std::string> derep_texts(const AfterJoin& A, const Postings& P, const ksp_edge* edges, const uint64_t n_edges) {
    std::vector<std::string> text(A.rep.size());
    for (size_t v = 0; v < A.rep.size(); ++v) {
        if (A.rep[v] == v) continue;
        const uint32_t e = A.via[v];
        if (e >= n_edges) throw std::runtime_error("dereplicate: the device named a record that does not exist");
        char buf[64];
        buf[ksp::format_float(buf, column_value(A.col, edges[e].shared, P.counts[edges[e].source_1], P.counts[edges[e].source_2]))] = 0;
        text[v] = buf;
    }
    return text;
}

// No host fix-up: at a threshold >= 0 a shared-0 row has the value 0 or NaN and never passes.  The device ranked the sources of
// the index; a row of .namesMap without one has no neighbour and follows them, in node order, as every node of degree 0 does.
void finish_derep(PairwiseJob& job, const Postings& P, const std::vector<std::string>& text, const std::vector<std::string>& name_of) {
    const AfterJoin& A = job.after;
    const uint64_t NN = name_of.size();
    std::vector<ksp::DerepRow> rows((size_t)NN);
    std::vector<uint8_t> seen((size_t)NN, 0);
    uint32_t with_neighbour = 0, reps = 0;
    for (uint32_t i = 0; i < (uint32_t)P.ids.size(); ++i) {
        ksp::check_row_nodes(P.ids[i], P.ids[A.rep[i]], NN);
        ksp::DerepRow& r = rows[P.ids[i] - 1];
        r.rep = P.ids[A.rep[i]] - 1;
        r.degree = A.degree[i];
        r.rank = A.node[i];
        r.text = text[i];
        seen[P.ids[i] - 1] = 1;
        with_neighbour += A.degree[i] != 0;
    }
    uint32_t next = with_neighbour;   // (index order is id order: the sources with a neighbour hold the ranks below this in both orders)
    for (uint64_t v = 0; v < NN; ++v) {
        if (!seen[v]) rows[v].rep = (uint32_t)v;
        if (rows[v].degree == 0) rows[v].rank = next++;
        reps += rows[v].rep == v;
    }
    ksp::write_derep_file(job.repr_out.empty() ? job.prefix + "_kSpider_dereplicated_" + job.dist + ".tsv" : job.repr_out, job.dist, rows, name_of);
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: dereplicated " << NN << " sources: " << A.derep.kept << " records kept, " << reps << " representatives, " << A.derep.dispatched
                  << " rounds and " << A.derep.tail << " in the tail" << std::endl;
}

// the order of the top-k definition on (value, place among all rows): value descending, a NaN below every number, lower place first
bool topk_before(const float vx, const uint64_t ix, const float vy, const uint64_t iy) {
    const bool nx = vx != vx, ny = vy != vy;
    if (nx != ny) return ny;
    if (!nx && vx != vy) return vx > vy;
    return ix < iy;
}

// The hits of every source, while the device's records are still here: the device's selection among its records, and the
// shared-0 rows (value 0, or NaN beside a source of 0 k-mers) merged in by the same order, the index of a row being its place
// in the (source_1, source_2) order of ALL rows — which keeps the device's records in the order of their own indices.
TopkHits device_topk(const AfterJoin& A, const Postings& P, const ksp_edge* edges, const uint64_t n_edges, const std::vector<ZeroRow>& zero_rows) {
    const uint32_t N = (uint32_t)P.ids.size(), k = A.k;
    TopkHits H;
    H.count.assign(N, 0);
    std::vector<std::vector<uint32_t>> zero_of;   // per source index: its shared-0 rows
    std::vector<uint64_t> zero_place;             // per shared-0 row: its place among all rows
    if (!zero_rows.empty()) {
        zero_of.resize(N);
        zero_place.resize(zero_rows.size());
        for (size_t z = 0; z < zero_rows.size(); ++z) {
            const ZeroRow& r = zero_rows[z];
            zero_of[r.a].push_back((uint32_t)z);
            zero_of[r.b].push_back((uint32_t)z);
            zero_place[z] = z + (uint64_t)(std::lower_bound(edges, edges + n_edges, r, [](const ksp_edge& e, const ZeroRow& q) {
                                               return e.source_1 != q.a ? e.source_1 < q.a : e.source_2 < q.b;
                                           }) - edges);
        }
    }
    auto place_of = [&](const uint32_t e) -> uint64_t {   // of a device record: the shared-0 rows before it are counted in
        if (zero_rows.empty()) return e;
        return e + (uint64_t)(std::lower_bound(zero_rows.begin(), zero_rows.end(), edges[e], [](const ZeroRow& q, const ksp_edge& x) {
                                  return q.a != x.source_1 ? q.a < x.source_1 : q.b < x.source_2;
                              }) - zero_rows.begin());
    };
    struct Cand { float v; uint64_t place; uint32_t nb; };
    std::vector<Cand> cand;
    for (uint32_t i = 0; i < N; ++i) {
        cand.clear();
        if (A.count[i] > k) throw std::runtime_error("topk: the device named more hits than were asked");
        for (uint32_t j = 0; j < A.count[i]; ++j) {
            const uint32_t e = A.index[(size_t)i * k + j];
            if (e >= n_edges || (edges[e].source_1 != i && edges[e].source_2 != i)) throw std::runtime_error("topk: the device named a record that is no entry of the source");
            const ksp_edge& x = edges[e];
            cand.push_back(Cand{column_value(A.col, x.shared, P.counts[x.source_1], P.counts[x.source_2]), place_of(e), x.source_1 == i ? x.source_2 : x.source_1});
        }
        if (!zero_rows.empty() && !zero_of[i].empty()) {
            for (const uint32_t z : zero_of[i]) {
                const ZeroRow& r = zero_rows[z];
                cand.push_back(Cand{column_value(A.col, 0, P.counts[r.a], P.counts[r.b]), zero_place[z], r.a == i ? r.b : r.a});
            }
            std::sort(cand.begin(), cand.end(), [](const Cand& x, const Cand& y) { return topk_before(x.v, x.place, y.v, y.place); });
            if (cand.size() > k) cand.resize(k);
        }
        H.count[i] = (uint32_t)cand.size();
        for (const Cand& c : cand) { H.neighbour.push_back(c.nb); H.value.push_back(c.v); }
    }
    return H;
}

// the file: the sources of the index are rows of .namesMap (checked before the first file); a row without a source has no hit
void finish_topk(PairwiseJob& job, const Postings& P, const TopkHits& H, const std::vector<std::string>& name_of, const uint64_t n_edges) {
    const AfterJoin& A = job.after;
    std::vector<uint32_t> count(name_of.size(), 0), neighbour;
    std::vector<std::string> text;
    for (uint32_t i = 0; i < (uint32_t)P.ids.size(); ++i) count[P.ids[i] - 1] = H.count[i];   // (index order is id order: the flat hits stay in place)
    for (size_t h = 0; h < H.neighbour.size(); ++h) {
        char buf[64];
        buf[ksp::format_float(buf, H.value[h])] = 0;
        neighbour.push_back(P.ids[H.neighbour[h]] - 1);
        text.push_back(buf);
    }
    ksp::write_topk_file(job.repr_out.empty() ? job.prefix + "_kSpider_topk_" + job.dist + ".tsv" : job.repr_out, job.dist, name_of, count, neighbour, text);
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: top " << A.k << " of " << n_edges << " records: " << neighbour.size() << " hits written; nodes selected by wave / workgroup / stream kernel: "
                  << A.topk.wave << " / " << A.topk.workgroup << " / " << A.topk.stream << std::endl;
}

// the value of every member's via record, while the device's records are still here (per source index; 0 without one)
std::vector<float> report_via_values(const AfterJoin& A, const Postings& P, const ksp_edge* edges, const uint64_t n_edges) {
    std::vector<float> value(A.member_rows.size(), 0.0f);
    for (size_t i = 0; i < A.member_rows.size(); ++i) {
        const uint32_t e = A.member_rows[i].via;
        if (e == 0xFFFFFFFFu) continue;
        if (e >= n_edges || (edges[e].source_1 != i && edges[e].source_2 != i)) throw std::runtime_error("cluster report: the device named a record that does not name the source");
        value[i] = column_value(A.col, edges[e].shared, P.counts[edges[e].source_1], P.counts[edges[e].source_2]);
    }
    return value;
}

// The device reported on its own records.  A shared-0 row (value 0, or NaN beside a source of 0 k-mers) is kept when it is a NaN
// or when cutoff * 100 <= 0 — the same test — and never reached the device: if one is kept, the report is made again by
// ksp_cluster_report_valued over all kept rows in (source_1, source_2) order, so that none is silently missing.  Then the rows
// of the sources become rows of .namesMap nodes (index order is id order; a name without a source is a singleton) and the files.
int finish_report(PairwiseJob& job, const Postings& P, const std::vector<ZeroRow>& zero_rows, const std::vector<ksp::EdgeRow>& rows, std::vector<float>& via_value,
                  const std::vector<std::string>& name_of, const int device) {
    AfterJoin& A = job.after;
    const uint32_t N = (uint32_t)P.ids.size(), none = 0xFFFFFFFFu;
    const uint64_t NN = name_of.size();
    float vcrit = 0;
    int mode = 0;
    ksp::cc_critical(A.cutoff, &vcrit, &mode);
    auto kept_zero = [&](const ZeroRow& z) { return passes_cut(column_value(A.col, 0, P.counts[z.a], P.counts[z.b]), vcrit, mode); };
    uint64_t n_kept = A.report.kept;
    if (std::any_of(zero_rows.begin(), zero_rows.end(), kept_zero)) {
        std::vector<uint32_t> ea, eb;
        std::vector<float> val;
        for (const ksp::EdgeRow& r : rows) {
            const uint32_t a = P.dense(r.source_1), b = P.dense(r.source_2);
            const float v = column_value(A.col, r.shared, P.counts[a], P.counts[b]);
            if (!passes_cut(v, vcrit, mode)) continue;
            ea.push_back(a); eb.push_back(b); val.push_back(v);
        }
        uint32_t n_clusters = 0;
        A.cluster_rows.assign((size_t)N + 1, ksp_cluster_row());
        A.member_rows.assign((size_t)N + 1, ksp_member_row());
        const int rc = ksp_cluster_report_valued(device, N, ea.data(), eb.data(), val.data(), ea.size(), A.cluster_rows.data(), &n_clusters, A.member_rows.data());
        if (rc != KSP_OK) return rc;
        A.cluster_rows.resize(n_clusters);
        A.member_rows.resize(N);
        via_value.assign(N, 0.0f);
        for (uint32_t i = 0; i < N; ++i)
            if (A.member_rows[i].via != none) via_value[i] = val[A.member_rows[i].via];
        n_kept = ea.size();
    }
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<ksp_member_row> member((size_t)NN);
    std::vector<std::string> via_text((size_t)NN);
    std::vector<int64_t> source_of((size_t)NN, -1);
    for (uint64_t v = 0; v < NN; ++v) member[v] = ksp_member_row{(uint32_t)v, 0u, 0, none, 0u};
    for (uint32_t i = 0; i < N; ++i) {
        const ksp_member_row& m = A.member_rows[i];
        const uint32_t v = P.ids[i] - 1;   // (every source is a row of .namesMap: checked before the first file)
        member[v] = ksp_member_row{P.ids[m.label] - 1, m.degree, m.strength, m.via, 0u};
        source_of[v] = i;
        if (m.via != none) {
            char buf[64];
            buf[ksp::format_float(buf, via_value[i])] = 0;
            via_text[v] = buf;
        }
    }
    std::vector<ksp_cluster_row> cluster;
    size_t next = 0;   // (the device's rows ascend by root, and so do their nodes)
    for (uint64_t v = 0; v < NN; ++v) {
        if (source_of[v] < 0) { cluster.push_back(ksp_cluster_row{(uint32_t)v, 1u, 0, 0, 0, nan, nan, (uint32_t)v, 0u}); continue; }
        if (member[v].label != v) continue;
        if (next >= A.cluster_rows.size() || A.cluster_rows[next].root != (uint32_t)source_of[v]) throw std::runtime_error("cluster report: the device's rows do not match its labels");
        ksp_cluster_row c = A.cluster_rows[next++];
        c.root = (uint32_t)v;
        c.medoid = P.ids[c.medoid] - 1;
        cluster.push_back(c);
    }
    ksp::write_report_files(job.prefix, job.dist, A.cutoff * 100.0, cluster, member, via_text, name_of);
    if (std::getenv("KSPIDER_VERBOSE")) {
        const ksp_cluster_row* big = nullptr;
        for (const ksp_cluster_row& c : cluster)
            if (!big || c.size > big->size) big = &c;
        std::cout << "kspider_amd: cluster report: " << n_kept << " records kept, " << cluster.size() << " clusters";
        if (big) {
            char buf[64] = "-";
            if (big->size > 1) std::snprintf(buf, sizeof buf, "%.6g", (double)big->edges / ((double)big->size * (big->size - 1.0) / 2.0));
            std::cout << ", the largest of " << big->size << " sources, density " << buf;
        }
        std::cout << std::endl;
    }
    return KSP_OK;
}

// The device's merges name source indices: index order is id order, so lo < hi and "the smallest member" survive the step to
// .namesMap nodes (id - 1).  A shared-0 row has q = 0 and takes no part: nothing to merge in on the host.
void finish_upgma(PairwiseJob& job, const Postings& P, const std::vector<std::string>& name_of) {
    AfterJoin& A = job.after;
    std::vector<ksp_upgma_row> rows = A.upgma_rows;
    for (ksp_upgma_row& r : rows) {
        r.lo = P.ids[r.lo] - 1;   // (every source is a row of .namesMap: checked before the first file)
        r.hi = P.ids[r.hi] - 1;
    }
    ksp::write_upgma_files(job.prefix, job.dist, rows, name_of, job.newick);
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: upgma: " << A.upgma.taking_part << " records taking part, " << A.upgma.first_pairs << " pairs, " << A.upgma.rounds
                  << " device rounds, merges " << A.upgma.device_merges << " on the device / " << A.upgma.host_merges << " by the host finish" << std::endl;
}

// Mirrors src/pairwise.cpp:123-276 phase by phase (the head of this file), with what job.after asks for between the join and the files.
int run_job(PairwiseJob& job) {
    AfterJoin& A = job.after;
    // $KSPIDER_TSV, read once, before anything is read or written: who makes the rows' text of the pairwise TSV
    bool device_tsv = false;
    std::string host_reason;   // why the host writes although the device was asked
    if (const char* tv = std::getenv("KSPIDER_TSV"); tv && *tv && std::strcmp(tv, "host") != 0) {
        if (std::strcmp(tv, "device") != 0) { ksp::set_error("pairwise: KSPIDER_TSV is 'host' or 'device', not '" + std::string(tv) + "'"); return KSP_E_ARG; }
        device_tsv = true;
    }
    const bool tsv_asked = device_tsv;
    std::shared_ptr<const std::vector<double>> ani_tab;
    if (job.ani) {   // before anything is read or written: the k-mer size (:44-46) and its table
        A.ksize = ksp::read_extra_ksize(job.prefix);
        ani_tab = ksp::ani_table(A.ksize);
    }
    ksp::IndexData ix;
    std::unordered_map<uint32_t, uint32_t> kmer_count;
    std::vector<std::string> derep_text, derep_names;
    int rc = load_inputs(job, ix, derep_names);
    if (rc != KSP_OK) return rc;

    // the postings before the first file: a group whose colour weights sum to 2^32 or more is refused with nothing written
    auto t0 = Clock::now();
    Postings P;
    index_postings(ix, P);
    const uint32_t N = (uint32_t)P.ids.size();
    const double t_transpose = since(t0);
    write_kmer_counts(job, ix, kmer_count);
    t0 = Clock::now();   // the timed region is the postings (t_transpose) plus everything from here to the rows
    const std::vector<int> devices = ksp::devices_from_env();
    ksp_stats st;
    auto t1 = Clock::now();
    if (A.kind != AfterJoin::kNone || device_tsv) {
        P.counts.resize(N);
        for (uint32_t i = 0; i < N; ++i) {
            auto it = kmer_count.find(P.ids[i]);
            P.counts[i] = it == kmer_count.end() ? 0u : it->second;   // (a missing group counts 0 k-mers, as operator[] of the reference yields)
        }
        A.kmer_counts = P.counts.data();
    }
    // The device writes the rows only where its text is exactly the host's: no shared-0 rows to splice in, no row with a NaN
    // (no source of 0 k-mers), and no ANI column, which reads the rows on the host.
    if (device_tsv && job.ani) { device_tsv = false; host_reason = "the ANI column reads the rows on the host"; }
    if (device_tsv && !P.zero_pairs.empty()) { device_tsv = false; host_reason = "rows of weight-0 colours are spliced in on the host"; }
    if (device_tsv && std::find(P.counts.begin(), P.counts.end(), 0u) != P.counts.end()) { device_tsv = false; host_reason = "a source has 0 k-mers"; }
    std::unique_ptr<ksp::PairwiseTsvPieces> pieces;   // (abandoned, and its .partial removed, on every way out before the commit)
    if (device_tsv) {
        pieces.reset(new ksp::PairwiseTsvPieces(job.prefix));
        A.want_text = true;
        A.ids = P.ids.data();
        A.text_sink = [&pieces](const char* text, const uint64_t n) {
            try {
                pieces->append(text, n);
            } catch (const std::exception& e) {
                ksp::set_error(e.what());
                return (int)KSP_E_IO;
            }
            return (int)KSP_OK;
        };
    }
    ksp_edge* pinned = nullptr;
    uint64_t n_edges = 0;
    rc = ksp::pairwise_postings_multi_cc(P.key_off.data(), P.post_src.data(), P.key_w.data(), (uint32_t)P.key_w.size(), N, devices.data(),
                                         (int)devices.size(), &pinned, &n_edges, &st, &A);
    std::unique_ptr<ksp_edge, void (*)(void*)> edges(pinned, ksp_free);   // (freed on every way out)
    const double t_device = since(t1);
    if (rc != KSP_OK) return rc;
    std::vector<ForestEdge> forest;
    if (A.kind == AfterJoin::kTree) forest = device_forest(A, P, edges.get(), n_edges);
    if (A.kind == AfterJoin::kDerep) derep_text = derep_texts(A, P, edges.get(), n_edges);
    std::vector<ksp::EdgeRow> rows;
    // (the device wrote the rows: there is no shared-0 row, and nobody reads `rows`)
    const std::vector<ZeroRow> zero_rows = device_tsv ? std::vector<ZeroRow>() : merge_rows(ix, P, A, edges.get(), n_edges, rows);
    const uint64_t n_rows = device_tsv ? n_edges : rows.size();
    TopkHits topk_hits;
    if (A.kind == AfterJoin::kTopk) topk_hits = device_topk(A, P, edges.get(), n_edges, zero_rows);
    std::vector<float> report_values;
    if (A.kind == AfterJoin::kReport) report_values = report_via_values(A, P, edges.get(), n_edges);
    edges.reset();
    if (job.ani && (rc = refuse_nan_rows(rows, kmer_count)) != KSP_OK) return rc;   // before anything of it is written
    std::cout << "pairwise hashmap construction: " << t_transpose + since(t0) << " secs" << std::endl;
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: postings from the colour index " << t_transpose << " s, device round trip " << t_device
                  << " s (stage 1 " << st.ms_build << " ms, join " << st.ms_join << " ms)" << std::endl;
    std::cout << "writing pairwise matrix to " << job.prefix << "_kSpider_pairwise.tsv" << std::endl;
    if (device_tsv) pieces->commit();
    else ksp::write_pairwise_tsv(job.prefix, rows, kmer_count, job.threads);
    if (tsv_asked && std::getenv("KSPIDER_VERBOSE")) {
        if (device_tsv) std::cout << "kspider_amd: pairwise TSV written by the device (" << A.text_bytes << " bytes of rows" << (A.edges_skipped ? ", the records stayed on the device" : "") << ")" << std::endl;
        else std::cout << "kspider_amd: pairwise TSV written by the host (" << host_reason << ")" << std::endl;
    }
    if (job.ani) {
        t0 = Clock::now();
        ksp::write_ani_column(job.prefix, rows, kmer_count, ani_tab->data(), job.threads);
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: ANI column " << since(t0) << " s" << std::endl;
    }
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: sources=" << N << " colour-entries=" << P.post_src.size() << " pairs=" << n_rows << std::endl;
    switch (A.kind) {
        case AfterJoin::kNone: break;
        case AfterJoin::kCut:
            if (std::getenv("KSPIDER_VERBOSE"))
                std::cout << "kspider_amd: cut at " << A.cutoff << " on column " << A.col << ": " << A.n_found << " edges found on the device, " << n_edges
                          << " kept; " << n_rows << " rows written" << std::endl;
            break;
        case AfterJoin::kRepr: finish_repr(job, P, zero_rows); break;
        case AfterJoin::kCluster: finish_cluster(job, P, zero_rows, n_edges, ani_tab ? ani_tab->data() : nullptr); break;
        case AfterJoin::kSweep: finish_sweep(job, P, zero_rows, n_edges); break;
        case AfterJoin::kTree: finish_tree(job, P, zero_rows, n_edges, forest); break;
        case AfterJoin::kDerep: finish_derep(job, P, derep_text, derep_names); break;
        case AfterJoin::kTopk: finish_topk(job, P, topk_hits, derep_names, n_edges); break;
        case AfterJoin::kUpgma: finish_upgma(job, P, derep_names); break;
        case AfterJoin::kReport: return finish_report(job, P, zero_rows, rows, report_values, derep_names, devices.empty() ? 0 : devices[0]);
    }
    return KSP_OK;
}

// run_job behind the C ABI: what it throws becomes ksp_last_error() (behind the entry point's name where it always named itself) and a code
int guarded(const char* entry, const bool prefixed, PairwiseJob& job) {
    try {
        return run_job(job);
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(entry) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        const std::string m = e.what();
        ksp::set_error(prefixed ? std::string(entry) + ": " + m : m);
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}
// column 3 / 4 / 5 of a containment distance's name (NULL or "": fallback), 0 for any other; *name: the name that was looked up
int dist_column(const char* dist_type, const char* fallback, std::string* name) {
    *name = dist_type && *dist_type ? dist_type : fallback;
    return *name == "min_cont" ? 3 : *name == "avg_cont" ? 4 : *name == "max_cont" ? 5 : 0;
}

}  // namespace

extern "C" int kspider_pairwise(const char* index_prefix, int user_threads) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise: index_prefix is NULL"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads);
    return guarded("kspider_pairwise", false, job);
}

extern "C" int kspider_pairwise_and_cluster(const char* index_prefix, int user_threads, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_cluster: index_prefix is NULL"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_cluster: distance '" + dt + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_cluster)");
        return KSP_E_ARG;
    }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kCluster, col);
    job.after.cutoff = cutoff;
    return guarded("kspider_pairwise_and_cluster", false, job);
}

extern "C" int kspider_pairwise_and_cluster_sweep(const char* index_prefix, int user_threads, const char* dist_type, const double* cutoffs,
                                                  uint32_t n_cutoffs) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_cluster_sweep: index_prefix is NULL"); return KSP_E_ARG; }
    if (!cutoffs || n_cutoffs < 1 || n_cutoffs > KSP_SWEEP_MAX_CUTOFFS) {
        ksp::set_error("kspider_pairwise_and_cluster_sweep: between 1 and " + std::to_string(KSP_SWEEP_MAX_CUTOFFS) + " cut-offs");
        return KSP_E_ARG;
    }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_cluster_sweep: distance '" + dt + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_cluster_sweep)");
        return KSP_E_ARG;
    }
    for (uint32_t i = 0; i < n_cutoffs; ++i)
        if (cutoffs[i] != cutoffs[i]) { ksp::set_error("kspider_pairwise_and_cluster_sweep: a cut-off is NaN"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kSweep, col);
    job.dist = dt;
    job.after.cutoffs = cutoffs;
    job.after.n_cutoffs = n_cutoffs;
    return guarded("kspider_pairwise_and_cluster_sweep", false, job);
}

extern "C" int kspider_pairwise_and_tree(const char* index_prefix, int user_threads, const char* dist_type, int newick) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_tree: index_prefix is NULL"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_tree: distance '" + dt + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_tree)");
        return KSP_E_ARG;
    }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kTree, col);
    job.dist = dt;
    job.newick = newick != 0;
    return guarded("kspider_pairwise_and_tree", true, job);
}

extern "C" int kspider_pairwise_and_upgma(const char* index_prefix, int user_threads, const char* dist_type, int newick) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_upgma: index_prefix is NULL"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_upgma: distance '" + dt + "' is not min_cont, avg_cont or max_cont (an average is one of containments in [0, 1])");
        return KSP_E_ARG;
    }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kUpgma, col);
    job.dist = dt;
    job.newick = newick != 0;
    return guarded("kspider_pairwise_and_upgma", true, job);
}

extern "C" int kspider_pairwise_and_repr(const char* index_prefix, int user_threads, const char* dist_type, double threshold, const char* out_path) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_repr: index_prefix is NULL"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error("kspider_pairwise_and_repr: the threshold is NaN"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "avg_cont", &dt);
    if (!col) { ksp::set_error("kspider_pairwise_and_repr: distance '" + dt + "' is not min_cont, avg_cont or max_cont"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kRepr, col);
    job.after.threshold = threshold;
    if (out_path) job.repr_out = out_path;
    return guarded("kspider_pairwise_and_repr", true, job);
}

extern "C" int kspider_pairwise_and_dereplicate(const char* index_prefix, int user_threads, const char* dist_type, double threshold, const char* out_path) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_dereplicate: index_prefix is NULL"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error("kspider_pairwise_and_dereplicate: the threshold is NaN"); return KSP_E_ARG; }
    if (threshold < 0) { ksp::set_error("kspider_pairwise_and_dereplicate: the threshold is negative (a row without shared k-mers would pass)"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "avg_cont", &dt);
    if (!col) { ksp::set_error("kspider_pairwise_and_dereplicate: distance '" + dt + "' is not min_cont, avg_cont or max_cont"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kDerep, col);
    job.dist = dt;
    job.after.threshold = threshold;
    if (out_path) job.repr_out = out_path;
    return guarded("kspider_pairwise_and_dereplicate", true, job);
}

extern "C" int kspider_pairwise_and_topk(const char* index_prefix, int user_threads, const char* dist_type, uint32_t k, const char* out_path) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_topk: index_prefix is NULL"); return KSP_E_ARG; }
    if (k == 0 || k > KSP_TOPK_MAX_K) { ksp::set_error("kspider_pairwise_and_topk: k is 1 .. " + std::to_string(KSP_TOPK_MAX_K)); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_topk: distance '" + dt + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_topk)");
        return KSP_E_ARG;
    }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kTopk, col);
    job.dist = dt;
    job.after.k = k;
    if (out_path) job.repr_out = out_path;
    return guarded("kspider_pairwise_and_topk", true, job);
}

extern "C" int kspider_pairwise_and_cluster_report(const char* index_prefix, int user_threads, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_cluster_report: index_prefix is NULL"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_and_cluster_report: distance '" + dt + "' is not min_cont, avg_cont or max_cont (a report sums containments in [0, 1])");
        return KSP_E_ARG;
    }
    if (!(cutoff >= 0 && cutoff <= 1)) { ksp::set_error("kspider_pairwise_and_cluster_report: the cut-off is not in [0, 1]"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kReport, col);
    job.dist = dt;
    job.after.cutoff = cutoff;
    return guarded("kspider_pairwise_and_cluster_report", true, job);
}

extern "C" int kspider_pairwise_cut(const char* index_prefix, int user_threads, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_cut: index_prefix is NULL"); return KSP_E_ARG; }
    std::string dt;
    const int col = dist_column(dist_type, "max_cont", &dt);
    if (!col) {
        ksp::set_error("kspider_pairwise_cut: distance '" + dt + "' is not min_cont, avg_cont or max_cont" + (dt == "ani" ? " (the ANI column as the cut is not offered)" : ""));
        return KSP_E_ARG;
    }
    if (!(cutoff >= 0.0 && cutoff <= 1.0)) {   // (kSpider cluster's -c: a float in [0, 1]; a NaN fails both compares)
        ksp::set_error("kspider_pairwise_cut: the cut-off is not in [0, 1]");
        return KSP_E_ARG;
    }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kCut, col);
    job.after.cutoff = cutoff;
    return guarded("kspider_pairwise_cut", true, job);
}

extern "C" int kspider_pairwise_ani(const char* index_prefix, int user_threads, int64_t scale) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_ani: index_prefix is NULL"); return KSP_E_ARG; }
    if (scale <= 0) { ksp::set_error("kspider_pairwise_ani: estimating ANI needs the sourmash scale (> 0)"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads);
    job.ani = true;
    return guarded("kspider_pairwise_ani", true, job);
}

extern "C" int kspider_pairwise_ani_and_cluster(const char* index_prefix, int user_threads, int64_t scale, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_ani_and_cluster: index_prefix is NULL"); return KSP_E_ARG; }
    if (scale <= 0) { ksp::set_error("kspider_pairwise_ani_and_cluster: estimating ANI needs the sourmash scale (> 0)"); return KSP_E_ARG; }
    PairwiseJob job(index_prefix, user_threads, AfterJoin::kCluster, 6);   // column 6: the ANI column
    job.ani = true;
    job.after.cutoff = cutoff;
    return guarded("kspider_pairwise_ani_and_cluster", true, job);
}

extern "C" int ksp_index_info(const char* index_prefix, uint64_t out[6]) {
    if (!index_prefix || !out) {
        ksp::set_error("ksp_index_info: NULL argument");
        return KSP_E_ARG;
    }
    try {
        ksp::IndexData ix;
        ksp::load_index(index_prefix, ix);
        uint64_t m = 0;
        for (auto& c : ix.colors) m += c.second.size();
        out[0] = ix.colors.size();
        out[1] = ix.kmer_slots.size();
        out[2] = ix.colors_count.size();
        out[3] = m;
        out[4] = (uint64_t)ix.kwidth;
        out[5] = ix.trailer ? 1 : 0;
        return KSP_OK;
    } catch (const std::exception& e) {
        ksp::set_error(e.what());
        return KSP_E_IO;
    }
}

extern "C" int ksp_format_float(float value, char* buf) { return buf ? ksp::format_float(buf, value) : 0; }

// (tests) ksp_format_float on n values at once, in the layout of ksp_debug_format_floats: h_text[16 * i ...] = the h_len[i] bytes of value i
extern "C" int ksp_debug_format_floats_host(const float* h_values, uint64_t n, char* h_text, uint32_t* h_len) {
    if (n && (!h_values || !h_text || !h_len)) { ksp::set_error("ksp_debug_format_floats_host: NULL argument"); return KSP_E_ARG; }
    char buf[32];
    for (uint64_t i = 0; i < n; ++i) {
        const int len = ksp::format_float(buf, h_values[i]);
        if (len < 0 || len > 16) { ksp::set_error("ksp_debug_format_floats_host: a text longer than 16 bytes"); return KSP_E_ARG; }
        std::memcpy(h_text + 16 * i, buf, (size_t)len);
        h_len[i] = (uint32_t)len;
    }
    return KSP_OK;
}

namespace kSpider {
void pairwise(std::string index_prefix, int user_threads) {
    if (kspider_pairwise(index_prefix.c_str(), user_threads) != KSP_OK) throw std::runtime_error(ksp_last_error());
}
}  // namespace kSpider
