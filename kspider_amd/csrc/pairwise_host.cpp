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
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <set>
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

namespace {

typedef std::chrono::high_resolution_clock Clock;
double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// dist_type != nullptr: also cluster (kSpider cluster, ks_clustering.py:63-137) from the edges while they are on the device
// ani: also write the ANI column of `pairwise --estimate-ani` (ks_pairwise.py:29-84; k from PREFIX.extra); dist_type "ani"
// then clusters on it
// repr: also rank the sources by their neighbour counts (apps/repr_sketches.cpp:27-33,38-43), likewise from the edges on the device
struct ReprOpts {
    int col = 4;
    double threshold = 0.20;
    std::string out_path;   // "": PREFIX_kSpider_repr_sketches.txt
};
// cut: only the rows that pass a containment cut are wanted (kspider_pairwise_cut): the edges are cut on the device, directly after the join
struct CutOpts {
    int col = 5;
    double cutoff = 0;
};
// sweep: also cluster at every cut-off of a ladder (kspider_pairwise_and_cluster_sweep), from one pass over the edges on the device
struct SweepOpts {
    int col = 5;
    std::string dist;
    const double* cutoffs = nullptr;
    uint32_t n_cutoffs = 0;
};
// tree: also write the single-linkage tree (kspider_pairwise_and_tree): the maximum spanning forest of the edges, found on the device
struct TreeOpts {
    int col = 5;
    std::string dist;
    bool newick = false;
};
int run_pairwise(const std::string& prefix, int user_threads, const char* dist_type = nullptr, double cutoff = 0, bool ani = false,
                 const ReprOpts* repr = nullptr, const CutOpts* cut = nullptr, const SweepOpts* sweep = nullptr, const TreeOpts* tree = nullptr) {
    int cc_col = 0, ksize = 0;
    std::shared_ptr<const std::vector<double>> ani_tab;
    if (ani) {   // before anything is read or written: the k-mer size (:44-46) and its table
        ksize = ksp::read_extra_ksize(prefix);
        ani_tab = ksp::ani_table(ksize);
    }
    if (dist_type) {
        const std::string dt = *dist_type ? dist_type : "max_cont";
        cc_col = dt == "min_cont" ? 3 : dt == "avg_cont" ? 4 : dt == "max_cont" ? 5 : dt == "ani" && ani ? 6 : 0;
        if (!cc_col) {
            ksp::set_error("kspider_pairwise_and_cluster: distance '" + dt + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_cluster)");
            return KSP_E_ARG;
        }
    }
    auto t0 = Clock::now();
    ksp::IndexData ix;
    ksp::load_index(prefix, ix);
    if (repr)   // the reference tool reads the ids with stoi: refused before any file is written
        for (auto& c : ix.colors)
            for (uint32_t g : c.second)
                if (g > 2147483647u) {
                    ksp::set_error("kspider_pairwise_and_repr: group id " + std::to_string(g) + " exceeds 2^31 - 1 (the reference tool reads ids as int)");
                    return KSP_E_LIMIT;
                }
    std::cout << "mapping colors to groups: " << since(t0) << " secs" << std::endl;
    t0 = Clock::now();
    std::cout << "parsing index colors: " << since(t0) << " secs" << std::endl;
    t0 = Clock::now();
    ksp::write_seq_to_kmers(prefix, ix);
    std::unordered_map<uint32_t, uint32_t> kmer_count;
    for (auto& s : ix.kmer_slots) kmer_count[s.first] = s.second;
    std::cout << "kmer counting: " << since(t0) << " secs" << std::endl;

    t0 = Clock::now();
    // dense source index = rank of the group ID, so that index order == ID order and the
    // engine's (i < j) is the reference's ascending(source_1, source_2) (:73-78, :218)
    uint32_t max_id = 0;
    for (auto& c : ix.colors)
        for (uint32_t g : c.second) max_id = std::max(max_id, g);
    std::vector<uint32_t> ids;
    std::vector<uint32_t> dense_of;          // direct table when the ID space is small enough
    if (max_id < (1u << 28)) {
        std::vector<uint8_t> seen((size_t)max_id + 1, 0);
        for (auto& c : ix.colors)
            for (uint32_t g : c.second) seen[g] = 1;
        dense_of.assign((size_t)max_id + 1, 0);
        for (uint32_t g = 0; g <= max_id; ++g)
            if (seen[g]) { dense_of[g] = (uint32_t)ids.size(); ids.push_back(g); }
        if (ix.colors.empty()) ids.clear();
    } else {
        for (auto& c : ix.colors) ids.insert(ids.end(), c.second.begin(), c.second.end());
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    }
    const uint32_t N = (uint32_t)ids.size();
    auto dense = [&](uint32_t g) -> uint32_t {
        return dense_of.empty() ? (uint32_t)(std::lower_bound(ids.begin(), ids.end(), g) - ids.begin()) : dense_of[g];
    };

    // The colour index IS an inverted index (colour -> sources, src/pairwise.cpp:128-170): hand it to the
    // engine as postings — no transposition into per-source runs, no sort and prune on the device.
    std::vector<std::pair<uint32_t, uint32_t>> zero_pairs;   // pairs touched only through weight-0 colours
    std::vector<uint64_t> wsum((size_t)N, 0);
    std::vector<uint64_t> key_off;
    std::vector<uint32_t> post_src, key_w;
    key_off.push_back(0);
    {
        size_t total = 0;
        for (auto& c : ix.colors) total += c.second.size() >= 2 ? c.second.size() : 0;
        post_src.reserve(total);
        key_off.reserve(ix.colors.size() + 1);
        key_w.reserve(ix.colors.size());
    }
    for (size_t ci = 0; ci < ix.colors.size(); ++ci) {
        auto& c = ix.colors[ci];
        uint32_t w = 0;
        if (!ix.colors_count.find(c.first, w)) w = 0;   // colorsCount[item.first] (:221): 0 when absent
        if (c.second.size() < 2) continue;          // a colour with one source produces no pair
        if (w == 0) {
            // the reference still creates the pair entries (with += 0): remember them
            for (size_t x = 0; x < c.second.size(); ++x)
                for (size_t y = x + 1; y < c.second.size(); ++y) {
                    uint32_t a = c.second[x], b = c.second[y];
                    if (a > b) std::swap(a, b);
                    if (a != b) zero_pairs.emplace_back(a, b);
                }
            continue;
        }
        for (uint32_t g : c.second) {
            const uint32_t di = dense(g);
            post_src.push_back(di);
            wsum[di] += w;
        }
        key_off.push_back(post_src.size());
        key_w.push_back(w);
    }
    for (uint32_t s = 0; s < N; ++s)
        if (wsum[s] >= (1ull << 32))
            throw std::runtime_error("kspider_amd: colour weights of group " + std::to_string(ids[s]) +
                                     " sum to >= 2^32 (32-bit pair counters would overflow)");
    const uint64_t E = post_src.size();
    // (a source cannot repeat inside a colour: flat_hash_set; two colours narrowing to the same uint32 id
    //  were resolved by load_index the way insert_or_assign does)

    const double t_transpose = since(t0);
    const std::vector<int> devices = ksp::devices_from_env();
    ksp_edge* edges = nullptr;
    uint64_t n_edges = 0;
    ksp_stats st;
    auto t1 = Clock::now();
    ksp::CcRequest cc;
    std::vector<uint32_t> cc_counts, cc_labels;
    ksp::ReprRequest rq;
    std::vector<uint32_t> rq_node, rq_count;
    ksp::CutRequest cq;
    ksp::SweepRequest sq;
    std::vector<uint32_t> sq_labels;
    std::vector<uint64_t> sq_kept;
    ksp::TreeRequest tq;
    std::vector<uint32_t> tq_index;
    if (cc_col || repr || cut || sweep || tree) {
        cc_counts.resize(N);
        for (uint32_t i = 0; i < N; ++i) {
            auto it = kmer_count.find(ids[i]);
            cc_counts[i] = it == kmer_count.end() ? 0u : it->second;   // (a missing group counts 0 k-mers, as operator[] of the reference yields)
        }
        cc.kmer_counts = cc_counts.data(); cc.col = cc_col; cc.cutoff = cutoff; cc.labels = &cc_labels; cc.ksize = ksize;
        if (repr) { rq.kmer_counts = cc_counts.data(); rq.col = repr->col; rq.threshold = repr->threshold; rq.node = &rq_node; rq.count = &rq_count; }
        if (cut) { cq.kmer_counts = cc_counts.data(); cq.col = cut->col; cq.cutoff = cut->cutoff; }
        if (sweep) {
            sq.kmer_counts = cc_counts.data(); sq.col = sweep->col; sq.cutoffs = sweep->cutoffs; sq.n_cutoffs = sweep->n_cutoffs;
            sq.labels = &sq_labels; sq.kept = &sq_kept;
        }
        if (tree) { tq.kmer_counts = cc_counts.data(); tq.col = tree->col; tq.index = &tq_index; }
    }
    int rc = ksp::pairwise_postings_multi_cc(key_off.data(), post_src.data(), key_w.data(), (uint32_t)key_w.size(), N,
                                             devices.data(), (int)devices.size(), &edges, &n_edges, &st, cc_col ? &cc : nullptr, repr ? &rq : nullptr,
                                             cut ? &cq : nullptr, sweep ? &sq : nullptr, tree ? &tq : nullptr);
    const double t_device = since(t1);
    if (rc != KSP_OK) return rc;
    // the forest's rows, while the device's records are still here: the value as the writer computes it, and its text
    auto column_value = [&](const int col, const uint64_t shared, const uint32_t a, const uint32_t b) {
        const float n1 = (float)cc_counts[a], n2 = (float)cc_counts[b];
        const float c12 = (float)shared / n2, c21 = (float)shared / n1;
        return col == 3 ? std::min(c12, c21) : col == 5 ? std::max(c12, c21) : (float)((double)(c12 + c21) / 2.0);
    };
    struct ForestEdge { uint32_t a, b; float v; };   // dense source indices
    std::vector<ForestEdge> forest;
    if (tree)
        for (const uint32_t e : tq_index) {
            if (e >= n_edges) { ksp_free(edges); throw std::runtime_error("tree: the device named a record that does not exist"); }
            forest.push_back(ForestEdge{edges[e].source_1, edges[e].source_2, column_value(tree->col, edges[e].shared, edges[e].source_1, edges[e].source_2)});
        }
    std::vector<ksp::EdgeRow> rows;
    rows.reserve(n_edges + zero_pairs.size());
    for (uint64_t i = 0; i < n_edges; ++i)
        rows.push_back(ksp::EdgeRow{ids[edges[i].source_1], ids[edges[i].source_2], edges[i].shared});
    ksp_free(edges);
    if (!zero_pairs.empty()) {
        std::sort(zero_pairs.begin(), zero_pairs.end());
        zero_pairs.erase(std::unique(zero_pairs.begin(), zero_pairs.end()), zero_pairs.end());
        const size_t nreal = rows.size();
        float vcrit = 0;
        int mode = 0;
        if (cut) ksp::cc_critical(cut->cutoff, &vcrit, &mode);
        const bool device_drops = mode || vcrit > 0;   // (otherwise every row passes: no value is negative)
        std::vector<std::pair<uint32_t, uint32_t>> unsure;   // kept as a shared-0 row, unless the device dropped a real row of the pair
        for (auto& zp : zero_pairs) {
            if (cut) {   // a row that exists only with shared_kmers = 0: the same test with the same vcrit / mode, on the host
                const float n1 = (float)cc_counts[dense(zp.first)], n2 = (float)cc_counts[dense(zp.second)];
                const float c12 = 0.0f / n2, c21 = 0.0f / n1;
                const float v = cut->col == 3 ? std::min(c12, c21) : cut->col == 5 ? std::max(c12, c21) : (float)((c12 + c21) / 2.0);
                if (!(mode ? v != v : !(v < vcrit))) continue;
            }
            auto it = std::lower_bound(rows.begin(), rows.begin() + nreal, zp,
                                       [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
                                           return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
                                       });
            if (it == rows.begin() + nreal || it->source_1 != zp.first || it->source_2 != zp.second) {
                if (cut && device_drops) unsure.push_back(zp);
                else rows.push_back(ksp::EdgeRow{zp.first, zp.second, 0});
            }
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
                if (!real[u]) rows.push_back(ksp::EdgeRow{unsure[u].first, unsure[u].second, 0});
        }
        std::sort(rows.begin(), rows.end(), [](const ksp::EdgeRow& a, const ksp::EdgeRow& b) {
            return a.source_1 != b.source_1 ? a.source_1 < b.source_1 : a.source_2 < b.source_2;
        });
    }
    if (ani)   // a row of a weight-0 colour with a source of 0 k-mers has a NaN containment, so no ANI: fail before writing
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
    std::cout << "pairwise hashmap construction: " << since(t0) << " secs" << std::endl;
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: postings from the colour index " << t_transpose << " s, device round trip " << t_device
                  << " s (stage 1 " << st.ms_build << " ms, join " << st.ms_join << " ms)" << std::endl;
    std::cout << "writing pairwise matrix to " << prefix << "_kSpider_pairwise.tsv" << std::endl;
    ksp::write_pairwise_tsv(prefix, rows, kmer_count, user_threads);
    if (ani) {
        t0 = Clock::now();
        ksp::write_ani_column(prefix, rows, kmer_count, ani_tab->data(), user_threads);
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: ANI column " << since(t0) << " s" << std::endl;
    }
    if (std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: sources=" << N << " colour-entries=" << E << " pairs=" << rows.size() << std::endl;
    if (cut && std::getenv("KSPIDER_VERBOSE"))
        std::cout << "kspider_amd: cut at " << cut->cutoff << " on column " << cut->col << ": " << cq.n_found << " edges found on the device, " << n_edges
                  << " kept; " << rows.size() << " rows written" << std::endl;
    if (repr) {
        // rows that only exist with shared_kmers = 0 (colours of weight 0) are rows of the TSV too: their value is 0 or NaN, which
        // passes a negative threshold only — the same text test, on the host, and the ranking redone with their counts
        std::vector<uint32_t> extra;
        for (auto& zp : zero_pairs) {
            auto it = std::lower_bound(rows.begin(), rows.end(), zp, [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
                return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
            });
            if (it == rows.end() || it->source_1 != zp.first || it->source_2 != zp.second || it->shared != 0) continue;
            const uint32_t a = dense(zp.first), b = dense(zp.second);
            const float n1 = (float)cc_counts[a], n2 = (float)cc_counts[b];
            const float c12 = 0.0f / n2, c21 = 0.0f / n1;
            const float v = repr->col == 3 ? std::min(c12, c21) : repr->col == 5 ? std::max(c12, c21) : (float)((c12 + c21) / 2.0);
            if (!ksp::repr_text_passes(v, repr->threshold)) continue;
            extra.push_back(a);
            extra.push_back(b);
        }
        if (!extra.empty()) {
            std::vector<uint32_t> degree((size_t)N, 0);
            for (size_t i = 0; i < rq_node.size(); ++i) degree[rq_node[i]] = rq_count[i];
            for (uint32_t v : extra) ++degree[v];
            rq_node.clear();
            for (uint32_t v = 0; v < N; ++v)
                if (degree[v]) rq_node.push_back(v);
            std::stable_sort(rq_node.begin(), rq_node.end(), [&](uint32_t x, uint32_t y) { return degree[x] > degree[y]; });
            rq_count.resize(rq_node.size());
            for (size_t i = 0; i < rq_node.size(); ++i) rq_count[i] = degree[rq_node[i]];
        }
        ksp::write_repr_file(repr->out_path.empty() ? prefix + "_kSpider_repr_sketches.txt" : repr->out_path, ids, rq_node.data(), rq_count.data(),
                             rq_node.size());
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: " << rq_node.size() << " sources with a neighbour ranked" << std::endl;
    }
    if (cc_col) {
        // the cluster file of `kSpider cluster` from the components the device found on the join's own edge records
        std::vector<std::string> name_of;
        ksp::read_names_map(prefix, name_of);
        const uint64_t NN = name_of.size();
        if (cc_labels.size() != N) cc_labels.assign(N, 0);   // (no edges at all: the device pass did not run)
        if (n_edges == 0) for (uint32_t i = 0; i < N; ++i) cc_labels[i] = i;
        // rows that only exist with shared_kmers = 0 (colours of weight 0) are rows of the TSV too: the same test, on the host
        if (!zero_pairs.empty()) {
            float vcrit = 0;
            int mode = 0;
            ksp::cc_critical(cutoff, &vcrit, &mode);
            std::vector<uint32_t> parent(cc_labels);
            auto find = [&](uint32_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
            bool merged = false;
            for (auto& zp : zero_pairs) {
                auto it = std::lower_bound(rows.begin(), rows.end(), zp, [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
                    return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
                });
                if (it == rows.end() || it->source_1 != zp.first || it->source_2 != zp.second || it->shared != 0) continue;   // (the pair also shares a weighted colour: an ordinary row)
                const uint32_t a = dense(zp.first), b = dense(zp.second);
                const float n1 = (float)cc_counts[a], n2 = (float)cc_counts[b];
                const float c12 = 0.0f / n2, c21 = 0.0f / n1;
                const float v = cc_col == 3 ? std::min(c12, c21) : cc_col == 5 ? std::max(c12, c21) : (float)((c12 + c21) / 2.0);
                bool kept = mode ? v != v : !(v < vcrit);
                if (cc_col == 6) {   // (the NaN rows were refused above)
                    double g = 0;
                    ksp::ani_of_row(std::min(c12, c21), std::max(c12, c21), ani_tab->data(), &g);
                    kept = !(g * 100.0 < cutoff * 100.0);
                }
                if (!kept) continue;
                const uint32_t ra = find(a), rb = find(b);
                if (ra != rb) { parent[std::max(ra, rb)] = std::min(ra, rb); merged = true; }
            }
            if (merged) for (uint32_t i = 0; i < N; ++i) cc_labels[i] = find(i);
        }
        std::vector<uint32_t> node_label((size_t)NN);
        for (uint64_t v = 0; v < NN; ++v) node_label[v] = (uint32_t)v;
        for (uint32_t i = 0; i < N; ++i) {
            if (cc_labels[i] == i) continue;   // (a root, or a source without a kept edge)
            const uint64_t a = ids[i], b = ids[cc_labels[i]];
            if (a < 1 || b < 1 || a > NN || b > NN)
                throw std::runtime_error("pairwise row names node " + std::to_string(std::max(a, b)) + " but .namesMap has " + std::to_string(NN) + " rows (ids must be 1..N)");
            node_label[a - 1] = (uint32_t)(b - 1);
        }
        ksp::write_cluster_file(prefix, cutoff * 100.0, node_label, name_of);
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: clusters from " << cc.n_kept << " edges that pass the cut" << std::endl;
    }
    if (sweep) {
        // the cluster file of `kSpider cluster` at every cut-off of the ladder, from the components the device found on the join's own edge records
        const uint32_t K = sweep->n_cutoffs;
        std::vector<std::string> name_of;
        ksp::read_names_map(prefix, name_of);
        const uint64_t NN = name_of.size();
        if (sq_labels.size() != (size_t)K * N || sq_kept.size() != K) {   // (the device pass did not run: every source is its own component)
            sq_labels.resize((size_t)K * N);
            for (size_t i = 0; i < sq_labels.size(); ++i) sq_labels[i] = (uint32_t)(i % N);
            sq_kept.assign(K, 0);
        }
        // rows that only exist with shared_kmers = 0 (colours of weight 0) are rows of the TSV too: the same test per cut-off, on the
        // host, and the row united into every rank it passes
        std::vector<std::pair<uint32_t, uint32_t>> zero_ends;
        std::vector<float> zero_val;
        for (auto& zp : zero_pairs) {
            auto it = std::lower_bound(rows.begin(), rows.end(), zp, [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
                return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
            });
            if (it == rows.end() || it->source_1 != zp.first || it->source_2 != zp.second || it->shared != 0) continue;   // (the pair also shares a weighted colour: an ordinary row)
            const uint32_t a = dense(zp.first), b = dense(zp.second);
            const float n1 = (float)cc_counts[a], n2 = (float)cc_counts[b];
            const float c12 = 0.0f / n2, c21 = 0.0f / n1;
            zero_ends.emplace_back(a, b);
            zero_val.push_back(sweep->col == 3 ? std::min(c12, c21) : sweep->col == 5 ? std::max(c12, c21) : (float)((c12 + c21) / 2.0));
        }
        std::vector<uint32_t> node_labels((size_t)K * NN);
        for (uint32_t i = 0; i < K; ++i) {
            uint32_t* lab = sq_labels.data() + (size_t)i * N;
            if (!zero_ends.empty()) {
                float vcrit = 0;
                int mode = 0;
                ksp::cc_critical(sweep->cutoffs[i], &vcrit, &mode);
                auto find = [&](uint32_t v) { while (lab[v] != v) { lab[v] = lab[lab[v]]; v = lab[v]; } return v; };
                bool merged = false;
                for (size_t z = 0; z < zero_ends.size(); ++z) {
                    const float v = zero_val[z];
                    if (!(mode ? v != v : !(v < vcrit))) continue;
                    ++sq_kept[i];
                    const uint32_t ra = find(zero_ends[z].first), rb = find(zero_ends[z].second);
                    if (ra != rb) { lab[std::max(ra, rb)] = std::min(ra, rb); merged = true; }
                }
                if (merged) for (uint32_t s = 0; s < N; ++s) lab[s] = find(s);
            }
            uint32_t* node_label = node_labels.data() + (size_t)i * NN;
            for (uint64_t v = 0; v < NN; ++v) node_label[v] = (uint32_t)v;
            for (uint32_t s = 0; s < N; ++s) {
                if (lab[s] == s) continue;   // (a root, or a source without a kept edge)
                const uint64_t a = ids[s], b = ids[lab[s]];
                if (a < 1 || b < 1 || a > NN || b > NN)
                    throw std::runtime_error("pairwise row names node " + std::to_string(std::max(a, b)) + " but .namesMap has " + std::to_string(NN) + " rows (ids must be 1..N)");
                node_label[a - 1] = (uint32_t)(b - 1);
            }
        }
        ksp::write_sweep_outputs(prefix, sweep->dist, sweep->cutoffs, K, node_labels.data(), sq_kept.data(), name_of);
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: clusters at " << K << " cut-offs from one pass over " << n_edges << " edges" << std::endl;
    }
    if (tree) {
        // the tree files of kspider_tree from the forest the device found on the join's own edge records
        std::vector<std::string> name_of;
        ksp::read_names_map(prefix, name_of);
        const uint64_t NN = name_of.size();
        // rows that only exist with shared_kmers = 0 (colours of weight 0) are rows of the TSV too: value 0 (a NaN with a source of 0
        // k-mers), united in on the host after the device's forest, in (source_1, source_2) order
        const size_t n_device = forest.size();
        for (auto& zp : zero_pairs) {   // (sorted above)
            auto it = std::lower_bound(rows.begin(), rows.end(), zp, [](const ksp::EdgeRow& r, const std::pair<uint32_t, uint32_t>& k) {
                return r.source_1 != k.first ? r.source_1 < k.first : r.source_2 < k.second;
            });
            if (it == rows.end() || it->source_1 != zp.first || it->source_2 != zp.second || it->shared != 0) continue;   // (the pair also shares a weighted colour: an ordinary row)
            const uint32_t a = dense(zp.first), b = dense(zp.second);
            forest.push_back(ForestEdge{a, b, column_value(tree->col, 0, a, b)});
        }
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
        auto find = [&](uint32_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
        std::vector<ksp::TreeRow> tree_rows;
        for (const uint32_t i : order) {
            const ForestEdge& fe = forest[i];
            const uint32_t ra = find(fe.a), rb = find(fe.b);
            if (ra == rb) continue;
            parent[std::max(ra, rb)] = std::min(ra, rb);
            const uint64_t a = ids[fe.a], b = ids[fe.b];
            if (a < 1 || b < 1 || a > NN || b > NN)
                throw std::runtime_error("pairwise row names node " + std::to_string(std::max(a, b)) + " but .namesMap has " + std::to_string(NN) + " rows (ids must be 1..N)");
            char buf[64];
            buf[ksp::format_float(buf, fe.v)] = 0;
            const double d = std::strtod(buf, nullptr);
            tree_rows.push_back(ksp::TreeRow{(uint32_t)(a - 1), (uint32_t)(b - 1), d * 100.0, d, buf});
        }
        ksp::write_tree_files(prefix, tree->dist, tree_rows, name_of, tree->newick);
        if (std::getenv("KSPIDER_VERBOSE")) std::cout << "kspider_amd: tree of " << tree_rows.size() << " merges from " << n_edges << " edges" << std::endl;
    }
    return KSP_OK;
}

}  // namespace

extern "C" int kspider_pairwise_and_tree(const char* index_prefix, int user_threads, const char* dist_type, int newick) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_tree: index_prefix is NULL"); return KSP_E_ARG; }
    TreeOpts opts;
    opts.dist = dist_type && *dist_type ? dist_type : "max_cont";
    opts.col = opts.dist == "min_cont" ? 3 : opts.dist == "avg_cont" ? 4 : opts.dist == "max_cont" ? 5 : 0;
    if (!opts.col) {
        ksp::set_error("kspider_pairwise_and_tree: distance '" + opts.dist + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_tree)");
        return KSP_E_ARG;
    }
    opts.newick = newick != 0;
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, nullptr, 0, false, nullptr, nullptr, nullptr, &opts);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_and_tree: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_pairwise_and_tree: ") + e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise(const char* index_prefix, int user_threads) {
    if (!index_prefix) {
        ksp::set_error("kspider_pairwise: index_prefix is NULL");
        return KSP_E_ARG;
    }
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_and_cluster(const char* index_prefix, int user_threads, const char* dist_type, double cutoff) {
    if (!index_prefix) {
        ksp::set_error("kspider_pairwise_and_cluster: index_prefix is NULL");
        return KSP_E_ARG;
    }
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, dist_type ? dist_type : "", cutoff);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_and_cluster: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_and_cluster_sweep(const char* index_prefix, int user_threads, const char* dist_type, const double* cutoffs,
                                                  uint32_t n_cutoffs) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_cluster_sweep: index_prefix is NULL"); return KSP_E_ARG; }
    if (!cutoffs || n_cutoffs < 1 || n_cutoffs > KSP_SWEEP_MAX_CUTOFFS) {
        ksp::set_error("kspider_pairwise_and_cluster_sweep: between 1 and " + std::to_string(KSP_SWEEP_MAX_CUTOFFS) + " cut-offs");
        return KSP_E_ARG;
    }
    SweepOpts opts;
    opts.dist = dist_type && *dist_type ? dist_type : "max_cont";
    opts.col = opts.dist == "min_cont" ? 3 : opts.dist == "avg_cont" ? 4 : opts.dist == "max_cont" ? 5 : 0;
    if (!opts.col) {
        ksp::set_error("kspider_pairwise_and_cluster_sweep: distance '" + opts.dist + "' is not min_cont, avg_cont or max_cont (ani needs the separate ANI column file: run kspider_cluster_sweep)");
        return KSP_E_ARG;
    }
    for (uint32_t i = 0; i < n_cutoffs; ++i)
        if (cutoffs[i] != cutoffs[i]) { ksp::set_error("kspider_pairwise_and_cluster_sweep: a cut-off is NaN"); return KSP_E_ARG; }
    opts.cutoffs = cutoffs;
    opts.n_cutoffs = n_cutoffs;
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, nullptr, 0, false, nullptr, nullptr, &opts);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_and_cluster_sweep: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_and_repr(const char* index_prefix, int user_threads, const char* dist_type, double threshold, const char* out_path) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_and_repr: index_prefix is NULL"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error("kspider_pairwise_and_repr: the threshold is NaN"); return KSP_E_ARG; }
    ReprOpts opts;
    const std::string dt = dist_type && *dist_type ? dist_type : "avg_cont";
    opts.col = dt == "min_cont" ? 3 : dt == "avg_cont" ? 4 : dt == "max_cont" ? 5 : 0;
    if (!opts.col) { ksp::set_error("kspider_pairwise_and_repr: distance '" + dt + "' is not min_cont, avg_cont or max_cont"); return KSP_E_ARG; }
    opts.threshold = threshold;
    if (out_path) opts.out_path = out_path;
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, nullptr, 0, false, &opts);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_and_repr: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_pairwise_and_repr: ") + e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_cut(const char* index_prefix, int user_threads, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_cut: index_prefix is NULL"); return KSP_E_ARG; }
    CutOpts opts;
    const std::string dt = dist_type && *dist_type ? dist_type : "max_cont";
    opts.col = dt == "min_cont" ? 3 : dt == "avg_cont" ? 4 : dt == "max_cont" ? 5 : 0;
    if (!opts.col) {
        ksp::set_error("kspider_pairwise_cut: distance '" + dt + "' is not min_cont, avg_cont or max_cont" + (dt == "ani" ? " (the ANI column as the cut is not offered)" : ""));
        return KSP_E_ARG;
    }
    if (!(cutoff >= 0.0 && cutoff <= 1.0)) {   // (kSpider cluster's -c: a float in [0, 1]; a NaN fails both compares)
        ksp::set_error("kspider_pairwise_cut: the cut-off is not in [0, 1]");
        return KSP_E_ARG;
    }
    opts.cutoff = cutoff;
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, nullptr, 0, false, nullptr, &opts);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_cut: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_pairwise_cut: ") + e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_ani(const char* index_prefix, int user_threads, int64_t scale) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_ani: index_prefix is NULL"); return KSP_E_ARG; }
    if (scale <= 0) { ksp::set_error("kspider_pairwise_ani: estimating ANI needs the sourmash scale (> 0)"); return KSP_E_ARG; }
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, nullptr, 0, true);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_ani: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_pairwise_ani: ") + e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
}

extern "C" int kspider_pairwise_ani_and_cluster(const char* index_prefix, int user_threads, int64_t scale, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_pairwise_ani_and_cluster: index_prefix is NULL"); return KSP_E_ARG; }
    if (scale <= 0) { ksp::set_error("kspider_pairwise_ani_and_cluster: estimating ANI needs the sourmash scale (> 0)"); return KSP_E_ARG; }
    try {
        return run_pairwise(index_prefix, user_threads < 1 ? 1 : user_threads, "ani", cutoff, true);
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_pairwise_ani_and_cluster: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_pairwise_ani_and_cluster: ") + e.what());
        const std::string m = e.what();
        return m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
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

namespace kSpider {
void pairwise(std::string index_prefix, int user_threads) {
    if (kspider_pairwise(index_prefix.c_str(), user_threads) != KSP_OK) throw std::runtime_error(ksp_last_error());
}
}  // namespace kSpider
