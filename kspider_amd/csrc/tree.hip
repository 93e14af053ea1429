// The single-linkage hierarchy of the containment graph: a MAXIMUM SPANNING FOREST of the join's edge records, found on the
// device by Boruvka rounds, and the host side that turns a forest into a merge table, a newick file and, later,
// the cluster file of any cut-off.
//
// Order of edges: a strict total order — the column value as a float, larger first, a NaN above every number (a NaN row is kept
// at every cut-off); ties by record index, lower first.  No value is negative, so the bit pattern of the float is monotone;
// (value bits, inverted index) packed into one 64-bit word makes "the best edge leaving a component" one 64-bit atomicMax.
// With a strict total order the forest is unique and the picks of a round can only form 2-cycles (two components picking the
// SAME record): a longer cycle would need every pick to be strictly better than the one before it, all the way round.
//   prep      k_tree_prep: edge_col_value once per record into a structure of arrays a[] / b[] / key[] (12 bytes per record)
//   round     clear best[] of every root; k_tree_offer: every edge whose endpoints carry different labels offers its word to
//             both labels; k_tree_pick: every root with an offer hooks onto the other side of its record (in a mutual pick
//             only the larger label hooks) and keeps the word: best[v] of a node that is no root any more is the record that
//             merged it, for good — nobody offers to a non-root and nobody clears it; k_tree_jump until a pass changes nothing
//   forest    the words of all non-roots, sorted descending: the merge order (NaN first, then value, then lower index)
// Every pass owns chunks of kTreeChunkEdges consecutive records per workgroup, as the containment cut does (cut.hip), and no
// workgroup ever waits on another.  The host drives and bounds every loop.  Every count, offset and index is 64-bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "cluster_inputs.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"
#include "tree_newick.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kTreeChunkEdges = KSP_TREE_CHUNK_EDGES;   // (the reasons for 2 048 records per 256 threads: cut.hip)
constexpr int kTreeThreads = 256;
constexpr int kTreeIters = (int)(kTreeChunkEdges / kTreeThreads);   // records per lane and chunk
constexpr int kTreeMaxJumps = 34;                                   // a chain of 2^32 hooked roots flattens in 32 passes; one more sees no change
constexpr u32 kNanKey = 0xFFFFFFFFu;
static_assert(kTreeIters * kTreeThreads == (int)kTreeChunkEdges, "a chunk is whole ballots");

// first record of wave `wave` in chunk `chunk`: wave w owns the records [w * 512, (w + 1) * 512) of its chunk
__device__ inline u64 tree_wave_base(const u64 chunk, const u32 wave) { return chunk * kTreeChunkEdges + (u64)wave * (kTreeIters * 64); }

// (key, record index) as one word: a larger word is a better edge; no word of a record is 0 (the index is below 2^32 - 1)
__device__ inline unsigned long long tree_word(const u32 key, const u64 e) { return ((unsigned long long)key << 32) | (u32)~(u32)e; }

// The column value of every record, once: its bit pattern (a NaN: the top) beside the two endpoints.
__global__ __launch_bounds__(kTreeThreads) void k_tree_prep(const ksp_edge* __restrict__ ed, const u64 n, const u64 n_chunks, const u32* __restrict__ cnt,
                                                             const int col, u32* __restrict__ a, u32* __restrict__ b, u32* __restrict__ key) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = tree_wave_base(chunk, wave);
        ksp_edge x[kTreeIters];
#pragma unroll
        for (int k = 0; k < kTreeIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e < n) x[k] = ed[e];
        }
#pragma unroll
        for (int k = 0; k < kTreeIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e >= n) continue;
            const float v = edge_col_value(x[k], cnt, col);
            a[e] = x[k].source_1;
            b[e] = x[k].source_2;
            key[e] = v != v ? kNanKey : __float_as_uint(v);
        }
    }
}

__global__ void k_tree_init(u32* __restrict__ parent, unsigned long long* __restrict__ best, const u32 n) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) { parent[v] = v; best[v] = 0; }
}
// best[] of every root back to "no offer"; the word of a non-root is the record that merged it and stays
__global__ void k_tree_clear(const u32* __restrict__ parent, unsigned long long* __restrict__ best, const u32 n) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n && parent[v] == v) best[v] = 0;
}

// Every edge between two different labels offers its word to both.  Every tree is a star here (the jump passes of the round
// before ran until one changed nothing), so parent[x] IS the label of x.  PRELOAD: a plain load and compare before the atomic —
// in a giant component nearly every offer loses against a word that is already there, and a lost offer then costs a load that
// hits the L2 and no atomic at all.  The load is a relaxed one of device scope, so it is served where the atomics are made and
// not by a line a CU fetched before them; a word only grows during this kernel, so a load that still sees an older word merely
// lets the atomic decide, as it would have anyway.
template <bool PRELOAD>
__global__ __launch_bounds__(kTreeThreads) void k_tree_offer(const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ key, const u64 n,
                                                              const u64 n_chunks, const u32* __restrict__ parent, unsigned long long* best) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = tree_wave_base(chunk, wave);
        u32 xa[kTreeIters], xb[kTreeIters], xk[kTreeIters];
#pragma unroll
        for (int k = 0; k < kTreeIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            xa[k] = xb[k] = xk[k] = 0;
            if (e < n) { xa[k] = a[e]; xb[k] = b[e]; xk[k] = key[e]; }
        }
#pragma unroll
        for (int k = 0; k < kTreeIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e >= n) continue;
            const u32 la = parent[xa[k]], lb = parent[xb[k]];
            if (la == lb) continue;   // (a record with source_1 == source_2 ends here too)
            const unsigned long long w = tree_word(xk[k], e);
            if (!PRELOAD || __hip_atomic_load(&best[la], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < w) atomicMax(&best[la], w);
            if (!PRELOAD || __hip_atomic_load(&best[lb], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < w) atomicMax(&best[lb], w);
        }
    }
}

// Every root with an offer hooks onto the label at the other end of its record; when that label picked the same record, only
// the larger of the two hooks.  Reads parent[] and best[], writes next[] (a whole new parent array: the host swaps the two), so
// no thread ever reads a label another thread of this kernel has already changed.  *chosen is set when a root hooked.
__global__ void k_tree_pick(const u32* __restrict__ a, const u32* __restrict__ b, const u32* __restrict__ parent, const unsigned long long* __restrict__ best,
                            u32* __restrict__ next, const u32 n, u32* __restrict__ chosen) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const u32 p = parent[v];
    u32 to = p;
    if (p == v) {
        const unsigned long long w = best[v];
        if (w) {
            const u32 e = ~(u32)w;
            const u32 la = parent[a[e]], lb = parent[b[e]];
            const u32 s = la == v ? lb : la;
            if (best[s] != w || v > s) { to = s; *chosen = 1; }
        }
    }
    next[v] = to;
}
__global__ void k_tree_jump(u32* __restrict__ parent, const u32 n, u32* __restrict__ changed) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const u32 p = parent[v], gp = parent[p];
    if (gp != p) { parent[v] = gp; *changed = 1; }
}

// workgroups of the edge passes: one per chunk up to 8 per CU, the rest by the chunk loop; $KSP_TREE_MAX_WORKGROUPS (tests)
int tree_grid(const u64 n_chunks, unsigned* grid) {
    ksp::WorkgroupCap g;
    if (const int rc = ksp::workgroup_cap("KSP_TREE_MAX_WORKGROUPS", "tree", g)) return rc;
    *grid = g.grid_of(n_chunks);
    return KSP_OK;
}

// what one call holds on the device (memory of the call's DeviceArena): 12 bytes per record, 16 bytes per node
struct TreeBufs {
    u32 *a = nullptr, *b = nullptr, *key = nullptr;   // the records as a structure of arrays
    u32 *parent = nullptr, *next = nullptr;           // the labels and the array the pick kernel writes; swapped every round
    unsigned long long* best = nullptr;               // per root: the best word offered this round; per non-root: the record that merged it
    u32* flags = nullptr;                             // [0] a record was chosen this round, [1] a jump pass changed a parent
};
int tree_alloc(const char* who, const u32 N, const u64 n, ksp::DeviceArena& A, TreeBufs& B) {
    int rc = KSP_OK;
    if ((rc = ksp::device_fits(who, 12ull * n + 16ull * N + 8, "12 per record, 16 per node"))) return rc;
    for (u32** p : {&B.a, &B.b, &B.key})
        if ((rc = A.alloc(p, (size_t)n))) return rc;
    for (u32** p : {&B.parent, &B.next})
        if ((rc = A.alloc(p, (size_t)N))) return rc;
    if ((rc = A.alloc(&B.best, (size_t)N)) || (rc = A.alloc(&B.flags, 2))) return rc;
    return KSP_OK;
}

// The rounds over B.a / B.b / B.key (n records, N nodes) on the CURRENT device; the forest's record indices in merge order to
// h_index, their number to *n_forest.  *rounds (may be NULL): the rounds that ran, the last, empty one included.
int tree_rounds(const u32 N, const u64 n, TreeBufs& B, const bool preload, u32* h_index, u32* n_forest, u32* rounds) {
    int rc = KSP_OK;
    unsigned ge = 1;
    const unsigned gn = (N + 255) / 256;
    const u64 n_chunks = (n + kTreeChunkEdges - 1) / kTreeChunkEdges;
    int max_rounds = 2;   // ceil(log2(N)) + 2: the components that still have a leaving edge at least halve every round, and the last round chooses nothing
    while ((1ull << (max_rounds - 2)) < (u64)N) ++max_rounds;
    u32 h_flags[2] = {1, 0};
    int round = 0;
    if ((rc = tree_grid(n_chunks, &ge))) return rc;
    hipLaunchKernelGGL(k_tree_init, dim3(gn), dim3(256), 0, nullptr, B.parent, B.best, N);
    KSP_TRY_HIP(hipGetLastError());
    for (; h_flags[0] && round < max_rounds; ++round) {
        KSP_TRY_HIP(hipMemsetAsync(B.flags, 0, 8, nullptr));
        if (round) hipLaunchKernelGGL(k_tree_clear, dim3(gn), dim3(256), 0, nullptr, (const u32*)B.parent, B.best, N);
        if (preload) hipLaunchKernelGGL(k_tree_offer<true>, dim3(ge), dim3(kTreeThreads), 0, nullptr, (const u32*)B.a, (const u32*)B.b, (const u32*)B.key, n, n_chunks, (const u32*)B.parent, B.best);
        else hipLaunchKernelGGL(k_tree_offer<false>, dim3(ge), dim3(kTreeThreads), 0, nullptr, (const u32*)B.a, (const u32*)B.b, (const u32*)B.key, n, n_chunks, (const u32*)B.parent, B.best);
        hipLaunchKernelGGL(k_tree_pick, dim3(gn), dim3(256), 0, nullptr, (const u32*)B.a, (const u32*)B.b, (const u32*)B.parent, (const unsigned long long*)B.best, B.next, N, B.flags);
        KSP_TRY_HIP(hipGetLastError());
        std::swap(B.parent, B.next);
        KSP_TRY_HIP(hipMemcpy(h_flags, B.flags, 4, hipMemcpyDeviceToHost));
        if (!h_flags[0]) continue;   // (nothing chosen: nothing hooked, every tree is still a star)
        // Increasing weights along a path hook a whole chain of roots in one round: flattened completely before the next one,
        // so that parent[x] is the label of x again
        h_flags[1] = 1;
        for (int pass = 0; h_flags[1] && pass < kTreeMaxJumps; ++pass) {
            KSP_TRY_HIP(hipMemsetAsync(B.flags + 1, 0, 4, nullptr));
            hipLaunchKernelGGL(k_tree_jump, dim3(gn), dim3(256), 0, nullptr, B.parent, N, B.flags + 1);
            KSP_TRY_HIP(hipMemcpy(h_flags + 1, B.flags + 1, 4, hipMemcpyDeviceToHost));
        }
        if (h_flags[1]) { ksp::set_error("tree: the hooked roots did not flatten in " + std::to_string(kTreeMaxJumps) + " jump passes"); rc = KSP_E_HIP; goto done; }
    }
    if (h_flags[0]) { ksp::set_error("tree: more than " + std::to_string(max_rounds) + " rounds"); rc = KSP_E_HIP; goto done; }
    if (rounds) *rounds = (u32)round;
    {   // the forest: the word of every non-root, best first
        std::vector<u32> parent(N);
        std::vector<unsigned long long> best(N);
        KSP_TRY_HIP(hipMemcpy(parent.data(), B.parent, (size_t)N * 4, hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipMemcpy(best.data(), B.best, (size_t)N * 8, hipMemcpyDeviceToHost));
        u64 m = 0;
        for (u32 v = 0; v < N; ++v)
            if (parent[v] != v) best[m++] = best[v];
        if (m > n || m + 1 > (u64)N) { ksp::set_error("tree: more forest edges than a forest has"); rc = KSP_E_HIP; goto done; }
        std::sort(best.begin(), best.begin() + (size_t)m, std::greater<unsigned long long>());
        for (u64 i = 0; i < m; ++i) h_index[i] = ~(u32)best[i];
        *n_forest = (u32)m;
    }
done:
    return rc;
}

int check_forest_args(const char* who, const u64 n_edges, const bool null_input, const u32* h_index, const u32* n_forest) {
    if (!n_forest || (n_edges && (null_input || !h_index))) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 records or more (a record's index is half of its 64-bit key)"); return KSP_E_LIMIT; }
    return KSP_OK;
}

}  // namespace

namespace ksp {
// ksp_edges_forest on the CURRENT device
int tree_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, uint32_t* h_index,
                         uint32_t* n_forest, const bool preload, uint32_t* rounds) {
    int rc = KSP_OK;
    if (rounds) *rounds = 0;
    if (n_edges == 0 || n_nodes == 0) { *n_forest = 0; return KSP_OK; }
    TreeBufs B;
    ksp::DeviceArena A;
    unsigned grid = 1;
    const u64 n_chunks = (n_edges + kTreeChunkEdges - 1) / kTreeChunkEdges;
    if ((rc = tree_alloc("tree", n_nodes, n_edges, A, B))) return rc;
    if ((rc = tree_grid(n_chunks, &grid))) return rc;
    hipLaunchKernelGGL(k_tree_prep, dim3(grid), dim3(kTreeThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_cnt, col, B.a, B.b, B.key);
    KSP_TRY_HIP(hipGetLastError());
    rc = tree_rounds(n_nodes, n_edges, B, preload, h_index, n_forest, rounds);
done:
    return rc;
}
}  // namespace ksp

extern "C" int ksp_edges_forest(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                uint32_t* h_index, uint32_t* n_forest) {
    if (const int rc = check_forest_args("ksp_edges_forest", n_edges, !d_edges || !d_kmer_counts, h_index, n_forest)) return rc;
    if (dist_col < 3 || dist_col > 5) { ksp::set_error("ksp_edges_forest: dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_edges_forest", device)) return rc;
    return ksp::tree_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, h_index, n_forest);
}

extern "C" int ksp_forest_ranked(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_rank, uint64_t n_edges,
                                 uint32_t* h_index, uint32_t* n_forest) {
    if (const int rc = check_forest_args("ksp_forest_ranked", n_edges, !h_a || !h_b || !h_rank, h_index, n_forest)) return rc;
    for (u64 e = 0; e < n_edges; ++e)
        if (h_a[e] >= n_nodes || h_b[e] >= n_nodes) { ksp::set_error("ksp_forest_ranked: node index out of range"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_forest_ranked", device)) return rc;
    if (n_edges == 0) { *n_forest = 0; return KSP_OK; }
    int rc = KSP_OK;
    TreeBufs B;
    ksp::DeviceArena A;
    if ((rc = tree_alloc("ksp_forest_ranked", n_nodes, n_edges, A, B))) return rc;
    KSP_TRY_HIP(hipMemcpy(B.a, h_a, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemcpy(B.b, h_b, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemcpy(B.key, h_rank, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    rc = tree_rounds(n_nodes, n_edges, B, true, h_index, n_forest, nullptr);
done:
    return rc;
}

// (tools/tree_times.py) HIP-event times of `reps` runs of ksp_edges_forest's device part over the same records: which 0 = as
// shipped (a plain load and compare before every atomic), 1 = the atomic alone.  Each time covers everything the call does on
// the device, its allocations and the copy of the forest to the host included.  ms[reps]; *rounds: the rounds of the last run.
extern "C" int ksp_debug_tree_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                    int which, int reps, float* ms, uint32_t* h_index, uint32_t* n_forest, uint32_t* rounds) {
    if (!ms || reps < 1 || which < 0 || which > 1 || !rounds || !n_nodes || dist_col < 3 || dist_col > 5) { ksp::set_error("ksp_debug_tree_times: bad argument"); return KSP_E_ARG; }
    if (const int rc = check_forest_args("ksp_debug_tree_times", n_edges, !d_edges || !d_kmer_counts, h_index, n_forest)) return rc;
    if (const int rc = ksp::set_device("ksp_debug_tree_times", device)) return rc;
    int rc = KSP_OK;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if ((rc = ksp::tree_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, h_index, n_forest, which == 0, rounds))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}

// ---- the host side: merge table, newick, cuts ---------------------------------------------------------------------------------

namespace {

// greater weight first, a NaN above every number
bool weight_before(const double x, const double y) {
    const bool nx = x != x, ny = y != y;
    if (nx || ny) return nx && !ny;
    return x > y;
}

}  // namespace

namespace ksp {
// PREFIX_kSpider_tree_<dist>.tsv and, with newick, PREFIX_kSpider_tree_<dist>.newick from the rows of a spanning forest (node
// indices; any order: sorted here by weight descending, NaN first, then (a, b)).  On a failure every file this call created is
// removed again.
void write_tree_files(const std::string& prefix, const std::string& dist, std::vector<TreeRow>& rows, const std::vector<std::string>& name_of, const bool newick) {
    const u64 N = name_of.size();
    std::sort(rows.begin(), rows.end(), [](const TreeRow& x, const TreeRow& y) {
        if (weight_before(x.weight, y.weight) || weight_before(y.weight, x.weight)) return weight_before(x.weight, y.weight);
        return x.a != y.a ? x.a < y.a : x.b < y.b;
    });
    std::string table = "source_1\tsource_2\t" + dist + "\tmerged_size\n";
    {
        TreeDsu dsu(N);
        for (const TreeRow& r : rows) {
            const u32 ra = dsu.find(r.a), rb = dsu.find(r.b);
            if (ra == rb) throw std::runtime_error("tree: the chosen rows hold a cycle");
            const u32 lo = std::min(ra, rb), hi = std::max(ra, rb);
            dsu.parent[hi] = lo;
            dsu.size[lo] += dsu.size[hi];
            table += std::to_string((u64)r.a + 1) + "\t" + std::to_string((u64)r.b + 1) + "\t" + r.text + "\t" + std::to_string(dsu.size[lo]) + "\n";
        }
    }
    auto exists = [](const std::string& path) { return (bool)std::ifstream(path); };
    const std::string tsv = prefix + "_kSpider_tree_" + dist + ".tsv", nwk = prefix + "_kSpider_tree_" + dist + ".newick";
    std::vector<std::string> created;
    try {
        if (!exists(tsv)) created.push_back(tsv);
        write_file_atomically(tsv, table);
        if (newick) {
            if (!exists(nwk)) created.push_back(nwk);
            std::ofstream f;
            PartialFiles files;
            files.open(nwk, f);
            write_newick(f, rows, name_of);
            files.commit();
        }
    } catch (...) {
        for (const std::string& path : created) std::remove(path.c_str());
        throw;
    }
}
}  // namespace ksp

extern "C" int kspider_tree(const char* index_prefix, const char* dist_type, int newick) {
    if (!index_prefix) { ksp::set_error("kspider_tree: index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (!col) { ksp::set_error("kspider_tree: unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)"); return KSP_E_ARG; }
    try {
        std::vector<std::string> name_of;
        std::vector<u32> ea, eb;
        std::vector<double> weight;
        std::vector<std::string> text;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double d, const std::string& t) {
            ksp::check_row_nodes(a, b, name_of.size());   // every row is an edge of the tree's graph
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            weight.push_back(d);
            text.push_back(t);
        });
        const u64 N = name_of.size(), n = ea.size();
        // doubles (and ANI values) do not fit the device's key: the distinct weights, sorted, become ranks; a NaN is the top one
        std::vector<double> distinct;
        for (const double w : weight)
            if (w == w) distinct.push_back(w);
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        std::vector<u32> rank((size_t)n);
        for (u64 e = 0; e < n; ++e)
            rank[(size_t)e] = weight[(size_t)e] != weight[(size_t)e] ? (u32)distinct.size() : (u32)(std::lower_bound(distinct.begin(), distinct.end(), weight[(size_t)e]) - distinct.begin());
        std::vector<u32> index((size_t)std::min<u64>(N ? N - 1 : 0, n) + 1);
        u32 n_forest = 0;
        const int rc = ksp_forest_ranked(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), rank.data(), n, index.data(), &n_forest);
        if (rc) return rc;
        std::vector<ksp::TreeRow> rows;
        for (u32 i = 0; i < n_forest; ++i) {
            const u32 e = index[i];
            double v = 0;
            parse_float(text[e], v);
            rows.push_back(ksp::TreeRow{ea[e], eb[e], weight[e], v, text[e]});
        }
        ksp::write_tree_files(prefix, dt, rows, name_of, newick != 0);
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_tree: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_tree: ") + e.what());
        return KSP_E_IO;
    }
}

extern "C" int kspider_cluster_from_tree(const char* index_prefix, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_cluster_from_tree: index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    if (!cluster_col(dt)) { ksp::set_error("kspider_cluster_from_tree: unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)"); return KSP_E_ARG; }
    const double threshold = cutoff * 100.0;   // (ks_clustering.py: cutoff = float(cutoff) * 100)
    try {
        std::vector<std::string> name_of;
        ksp::read_names_map(prefix, name_of);
        const u64 N = name_of.size();
        const std::string path = prefix + "_kSpider_tree_" + dt + ".tsv";
        std::ifstream f(path);
        if (!f) throw std::runtime_error("cannot open " + path);
        TreeDsu dsu(N);
        std::string line;
        std::vector<std::string> p;
        std::getline(f, line);   // header
        while (std::getline(f, line)) {
            split_tabs(strip(line), p);
            long long a, b;
            double d;
            if (p.size() < 3 || !parse_id(p[0], a) || !parse_id(p[1], b) || !parse_float(p[2], d)) throw std::runtime_error("malformed row in " + path);
            ksp::check_row_nodes(a, b, N);
            if (d * 100.0 < threshold) continue;   // the row test of kspider_cluster on the same text (a NaN is not below anything: kept)
            const u32 ra = dsu.find((u32)(a - 1)), rb = dsu.find((u32)(b - 1));
            if (ra != rb) dsu.parent[std::max(ra, rb)] = std::min(ra, rb);
        }
        std::vector<u32> label((size_t)N);
        for (u64 v = 0; v < N; ++v) label[(size_t)v] = dsu.find((u32)v);
        ksp::write_cluster_file(prefix, threshold, label, name_of);
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_cluster_from_tree: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_cluster_from_tree: ") + e.what());
        return KSP_E_IO;
    }
}
