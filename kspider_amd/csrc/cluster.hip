// kspider_cluster(): the reference's `kSpider cluster` — pykSpider/kSpider2/ks_clustering.py:63-137 — with the
// connected components computed on the GPU.
//
// What the reference does (restated, nothing copied):
//   * nodes: one per row of PREFIX.namesMap (:56-61; first line skipped, "<id> <name>" split on blanks);
//     an edge names its nodes by INDEX = source id - 1 (:99-100), the output names a node by id = index + 1
//     (:135) — so the ids have to be 1..N, as the reference's indexers write them;
//   * edges: every row of PREFIX_kSpider_pairwise.tsv whose column dist_col (min_cont 3, avg_cont 4,
//     max_cont 5; ani: the one column of PREFIX_kSpider_pairwise.ani_col.tsv) parsed as a float and
//     multiplied by 100 is NOT below cutoff * 100 (:101-105; a NaN is never below: kept);
//   * rustworkx.connected_components, one output line per component: the names joined by ',' (:121-137),
//     singletons included, into PREFIX_kSpider_clusters_<cutoff*100>%.tsv (the number printed as Python
//     prints a float: shortest round-trip digits, ".0" on integers).
// Two deliberate differences, both stated in INTEGRATION.md: the reference loses every 10 000 001st kept edge
// (:107-113: the edge that finds the batch full is dropped with the flush — which edge that is depends on its
// hash-map row order); all edges are kept here.  And the order of the lines / of the names inside a line is
// rustworkx's set order there; here components come in order of their smallest node, members ascending.
//
// Device side: min-label hooking + pointer jumping (every parent[] only ever decreases, parent[v] <= v): when
// nothing changes any more every tree is a star whose root is the smallest node of its component.
#include <algorithm>
#include <charconv>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "ani.h"
#include "cc_kernels.hip.h"
#include "cluster_inputs.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

// The same pass straight over the join's edge records (ksp_edge, device memory): an edge counts when its containment
// column is not below the cut (cc_edge_kept, edge_cut.hip.h: one compare against the critical float of ksp::cc_critical).
// strict_nodes > 0 (the cluster report, report.hip): a record that names a node >= strict_nodes is ignored before anything is read
// through it, and so is a self pair, whatever its value — it never changes a component, so the labels are the same either way.
__global__ void k_cc_hook_edges(const ksp_edge* __restrict__ ed, u64 m, const u32* __restrict__ cnt, const int col, const float vcrit,
                                const int mode, const u32 strict_nodes, u32* __restrict__ parent, u32* __restrict__ changed,
                                unsigned long long* __restrict__ kept) {
    unsigned long long mine = 0;
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (u64)gridDim.x * blockDim.x) {
        const ksp_edge x = ed[e];
        if (strict_nodes && (x.source_1 >= strict_nodes || x.source_2 >= strict_nodes || x.source_1 == x.source_2)) continue;
        if (!cc_edge_kept(x, cnt, col, vcrit, mode)) continue;
        ++mine;
        const u32 pu = parent[x.source_1], pv = parent[x.source_2];
        if (pu == pv) continue;
        const u32 hi = pu > pv ? pu : pv, lo = pu > pv ? pv : pu;
        if (atomicMin(&parent[hi], lo) > lo) *changed = 1;
    }
    if (kept && mine) atomicAdd(kept, mine);
}

// The ANI of `kSpider pairwise --estimate-ani` (ani.h) on the join's edge records: columns 3 and 5 computed as
// cc_edge_kept computes them (the writer's single-precision maths, std::min / std::max NaN semantics), then the
// 6-digit decimal of each and one gather per column from the table the host filled.  A NaN column has no ANI.
__device__ inline void edge_min_max(const ksp_edge& x, const u32* __restrict__ cnt, float* mn, float* mx) {
    const float n1 = (float)cnt[x.source_1], n2 = (float)cnt[x.source_2];
    const float c12 = (float)x.shared / n2, c21 = (float)x.shared / n1;
    *mn = c21 < c12 ? c21 : c12;   // std::min(c12, c21)
    *mx = c12 < c21 ? c21 : c12;   // std::max(c12, c21)
}
__global__ void k_edges_ani(const ksp_edge* __restrict__ ed, u64 m, const u32* __restrict__ cnt, const double* __restrict__ table,
                            double* __restrict__ ani, u32* __restrict__ nan_seen) {
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (u64)gridDim.x * blockDim.x) {
        float mn, mx;
        edge_min_max(ed[e], cnt, &mn, &mx);
        double v;
        if (!ksp::ani_of_row(mn, mx, table, &v)) { v = __builtin_nan(""); *nan_seen = 1; }
        ani[e] = v;
    }
}
// The ANI cut, evaluated once per edge rather than once per hooking round: bit e of keep[] says edge e counts, i.e.
// float(repr(ani)) * 100 is not below cutoff * 100 (ks_clustering.py:101-105; repr round-trips, so that is the double
// compare below, thr = cutoff * 100.0).  A wave takes 64 consecutive edges and writes their 64 bits as one word (the
// loop bound is uniform over the wave: base is a multiple of 64, so every lane takes part in the ballot).
__global__ void k_ani_keep(const ksp_edge* __restrict__ ed, u64 m, const u32* __restrict__ cnt, const double* __restrict__ table,
                           const double thr, unsigned long long* __restrict__ keep, u32* __restrict__ nan_seen,
                           unsigned long long* __restrict__ kept) {
    const u32 lane = threadIdx.x & 63;
    unsigned long long mine = 0;
    for (u64 base = (u64)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < m; base += (u64)gridDim.x * blockDim.x) {
        const u64 e = base + lane;
        bool k = false;
        if (e < m) {
            float mn, mx;
            edge_min_max(ed[e], cnt, &mn, &mx);
            double v;
            if (!ksp::ani_of_row(mn, mx, table, &v)) *nan_seen = 1;
            else k = !(v * 100.0 < thr);
        }
        const unsigned long long bits = __ballot(k);
        if (lane == 0) keep[base >> 6] = bits;
        mine += k ? 1 : 0;
    }
    if (mine) atomicAdd(kept, mine);
}
// k_cc_hook_edges over the edges whose bit in keep[] is set
__global__ void k_cc_hook_kept(const ksp_edge* __restrict__ ed, u64 m, const unsigned long long* __restrict__ keep, u32* __restrict__ parent,
                               u32* __restrict__ changed) {
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < m; e += (u64)gridDim.x * blockDim.x) {
        if (!((keep[e >> 6] >> (e & 63)) & 1ull)) continue;
        const ksp_edge x = ed[e];
        const u32 pu = parent[x.source_1], pv = parent[x.source_2];
        if (pu == pv) continue;
        const u32 hi = pu > pv ? pu : pv, lo = pu > pv ? pv : pu;
        if (atomicMin(&parent[hi], lo) > lo) *changed = 1;
    }
}

}  // namespace

extern "C" int ksp_components(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, uint64_t n_edges,
                              uint32_t* h_label) {
    if ((n_edges && (!h_a || !h_b)) || (n_nodes && !h_label)) { ksp::set_error("ksp_components: NULL argument"); return KSP_E_ARG; }
    for (u64 e = 0; e < n_edges; ++e)
        if (h_a[e] >= n_nodes || h_b[e] >= n_nodes) { ksp::set_error("ksp_components: node index out of range"); return KSP_E_ARG; }
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr, *d_parent = nullptr, *d_changed = nullptr;
    u32 h_changed = 1;
    if ((rc = ksp::set_device("ksp_components", device))) return rc;
    if (n_nodes == 0) return KSP_OK;
    if ((rc = A.alloc(&d_parent, (size_t)n_nodes)) || (rc = A.alloc(&d_changed, 1))) return rc;
    if (n_edges && (rc = ksp::upload_pairs(A, h_a, h_b, n_edges, &d_a, &d_b))) return rc;
    {
        const unsigned gn = (n_nodes + 255) / 256;
        const unsigned ge = (unsigned)std::min<u64>((n_edges + 255) / 256, 1u << 16);
        hipLaunchKernelGGL(k_cc_init, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes);
        // every round at least halves the depth of every tree and merges what an edge connects: O(log n) rounds;
        // the bound only guards against a defect
        for (int round = 0; n_edges && h_changed && round < 10000; ++round) {
            KSP_TRY_HIP(hipMemsetAsync(d_changed, 0, 4, nullptr));
            hipLaunchKernelGGL(k_cc_hook, dim3(ge), dim3(256), 0, nullptr, d_a, d_b, n_edges, d_parent, d_changed);
            hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes, d_changed);
            hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes, d_changed);
            KSP_TRY_HIP(hipMemcpy(&h_changed, d_changed, 4, hipMemcpyDeviceToHost));
        }
        if (n_edges && h_changed) { ksp::set_error("ksp_components: did not converge"); rc = KSP_E_HIP; goto done; }
        KSP_TRY_HIP(hipMemcpy(h_label, d_parent, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    }
done:
    return rc;
}

namespace ksp {
// The reference keeps a row when float(text of the column) * 100 is not below cutoff * 100 (ks_clustering.py:101-105),
// the text being the float printed with 6 significant digits (src/pairwise.cpp:266-273 = ksp::format_float).  Printing,
// parsing and the multiplication are all monotone, so the rows kept are exactly those whose float is not below ONE
// critical float: found here by bisection over the non-negative floats (their bit patterns are ordered).
// mode 0: keep v when !(v < *vcrit);  mode 1: no finite value and no infinity passes — only NaN rows are kept.
void cc_critical(const double cutoff, float* vcrit, int* mode) {
    const double threshold = cutoff * 100.0;
    auto passes = [&](const uint32_t bits) {
        float v;
        std::memcpy(&v, &bits, 4);
        char buf[64];
        const int n = ksp_format_float(v, buf);
        buf[n] = 0;
        const double d = std::strtod(buf, nullptr) * 100.0;
        return !(d < threshold);
    };
    const uint32_t inf_bits = 0x7F800000u;
    *mode = 0;
    if (!passes(inf_bits)) { *mode = 1; *vcrit = 0; return; }
    uint32_t lo = 0, hi = inf_bits;   // the smallest pattern that passes lies in [lo, hi]; hi passes
    if (passes(0)) hi = 0;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (passes(mid)) hi = mid; else lo = mid + 1;
    }
    std::memcpy(vcrit, &hi, 4);
}

// the ANI table of ksize (ani.h) in device memory of the current device, owned by the arena
static int upload_ani_table(const int ksize, DeviceArena& A, double** d_table) {
    int rc = KSP_OK;
    *d_table = nullptr;
    if (ksize < 1) { set_error("ANI: k-mer size < 1"); return KSP_E_ARG; }
    std::shared_ptr<const std::vector<double>> t;
    try {
        t = ani_table(ksize);
    } catch (const std::exception&) {
        set_error("ANI: cannot build the table on the host (out of memory?)");
        return KSP_E_LIMIT;
    }
    if ((rc = A.alloc(d_table, (size_t)kAniTableSize))) return rc;
    KSP_TRY_HIP(hipMemcpy(*d_table, t->data(), (size_t)kAniTableSize * sizeof(double), hipMemcpyHostToDevice));
done:
    return rc;
}

// The rounds of hooking and pointer jumping over d_parent (n_nodes labels in device memory, initialised by k_cc_init or by the
// caller), until nothing changes: the labels stay on the device.  d_changed: 4 words of device memory, [0] changed, [2..3]
// the kept records of the first round (*n_kept, may be NULL; records only).
int cc_rounds_on_device(const CcRounds& R, const uint32_t n_nodes, const uint64_t n_edges, uint32_t* d_parent, uint32_t* d_changed, uint64_t* n_kept) {
    int rc = KSP_OK;
    u32 h_changed = 1;
    unsigned long long* const d_kept = reinterpret_cast<unsigned long long*>(d_changed + 2);
    const unsigned gn = (n_nodes + 255) / 256;
    const unsigned ge = (unsigned)std::min<u64>((n_edges + 255) / 256, 1u << 16);
    // every round at least halves the depth of every tree and merges what an edge connects: O(log n) rounds; the bound only
    // guards against a defect
    for (int round = 0; n_edges && h_changed && round < 10000; ++round) {
        KSP_TRY_HIP(hipMemsetAsync(d_changed, 0, 16, nullptr));
        if (R.keep)
            hipLaunchKernelGGL(k_cc_hook_kept, dim3(ge), dim3(256), 0, nullptr, R.ed, n_edges, R.keep, d_parent, d_changed);
        else if (R.ed)
            hipLaunchKernelGGL(k_cc_hook_edges, dim3(ge), dim3(256), 0, nullptr, R.ed, n_edges, R.cnt, R.col, R.vcrit, R.mode, R.strict ? n_nodes : 0u, d_parent,
                               d_changed, round == 0 ? d_kept : nullptr);
        else
            hipLaunchKernelGGL(k_cc_hook, dim3(ge), dim3(256), 0, nullptr, R.a, R.b, n_edges, d_parent, d_changed);
        hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes, d_changed);
        hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes, d_changed);
        KSP_TRY_HIP(hipMemcpy(&h_changed, d_changed, 4, hipMemcpyDeviceToHost));
        if (round == 0 && n_kept && R.ed && !R.keep) { unsigned long long k = 0; KSP_TRY_HIP(hipMemcpy(&k, d_kept, 8, hipMemcpyDeviceToHost)); *n_kept = k; }
    }
    if (n_edges && h_changed) { set_error("components: did not converge"); rc = KSP_E_HIP; }
done:
    return rc;
}
// d_parent[v] = v: every node its own component (the start of cc_rounds_on_device)
int cc_init_on_device(const uint32_t n_nodes, uint32_t* d_parent) {
    if (n_nodes) hipLaunchKernelGGL(k_cc_init, dim3((n_nodes + 255) / 256), dim3(256), 0, nullptr, d_parent, n_nodes);
    KSP_HIP(hipGetLastError());
    return KSP_OK;
}

// connected components of the kept edges among `d_edges` (device memory, on the current device); see ksp_components_edges
int cc_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double cutoff,
                       uint32_t* h_label, uint64_t* n_kept, int ksize) {
    int rc = KSP_OK;
    DeviceArena A;
    u32 *d_parent = nullptr, *d_changed = nullptr;   // d_changed: [0] changed, [1] NaN ANI seen, [2..3] kept edges
    unsigned long long* d_kept = nullptr;
    double* d_table = nullptr;
    unsigned long long* d_keep = nullptr;   // ANI: one bit per edge, the cut evaluated once
    float vcrit = 0;
    int mode = 0;
    if (col != 6) cc_critical(cutoff, &vcrit, &mode);
    if (n_kept) *n_kept = 0;
    if (n_nodes == 0) return KSP_OK;
    if ((rc = A.alloc(&d_parent, (size_t)n_nodes)) || (rc = A.alloc(&d_changed, 4))) return rc;
    d_kept = reinterpret_cast<unsigned long long*>(d_changed + 2);
    {
        const unsigned gn = (n_nodes + 255) / 256;
        hipLaunchKernelGGL(k_cc_init, dim3(gn), dim3(256), 0, nullptr, d_parent, n_nodes);
        if (col == 6 && n_edges) {   // the ANI cut of every edge, once: a bit per edge
            if ((rc = upload_ani_table(ksize, A, &d_table))) goto done;
            if ((rc = A.alloc(&d_keep, (size_t)((n_edges + 63) / 64)))) goto done;
            KSP_TRY_HIP(hipMemsetAsync(d_changed, 0, 16, nullptr));
            hipLaunchKernelGGL(k_ani_keep, dim3((unsigned)std::min<u64>((n_edges + 255) / 256, 2048)), dim3(256), 0, nullptr, d_edges, n_edges, d_cnt,
                               d_table, cutoff * 100.0, d_keep, d_changed + 1, d_kept);
            KSP_TRY_HIP(hipGetLastError());
            u32 head[4] = {0, 0, 0, 0};   // [1] NaN seen, [2..3] kept edges
            KSP_TRY_HIP(hipMemcpy(head, d_changed, 16, hipMemcpyDeviceToHost));
            if (head[1]) { set_error("components: an edge has a NaN containment (0 shared k-mers of a source with 0 k-mers): it has no ANI"); rc = KSP_E_ARG; goto done; }
            if (n_kept) { unsigned long long k; std::memcpy(&k, head + 2, 8); *n_kept = k; }
            (void)A.release(d_table);   // (not held through the rounds)
        }
        {
            CcRounds R;
            R.ed = d_edges; R.keep = d_keep; R.cnt = d_cnt; R.col = col; R.vcrit = vcrit; R.mode = mode;
            if ((rc = cc_rounds_on_device(R, n_nodes, n_edges, d_parent, d_changed, col != 6 ? n_kept : nullptr))) goto done;
        }
        KSP_TRY_HIP(hipMemcpy(h_label, d_parent, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    }
done:
    return rc;
}

// one line per component — in order of their smallest node, members ascending — into `out` (ks_clustering.py:121-137, 150-163);
// label[v] = smallest node of v's component, names by node index
void write_cluster_file_as(const std::string& out, const std::vector<u32>& label, const std::vector<std::string>& name_of) {
    const u64 N = label.size();
    std::vector<u32> count((size_t)N + 1, 0), order((size_t)N);
    for (u64 v = 0; v < N; ++v) ++count[label[v] + 1];
    for (u64 v = 0; v < N; ++v) count[v + 1] += count[v];
    {
        std::vector<u32> cur(count.begin(), count.end() - 1);
        for (u64 v = 0; v < N; ++v) order[cur[label[v]]++] = (u32)v;
    }
    std::ofstream f;
    PartialFiles files;
    files.open(out, f);
    for (u64 r = 0; r < N; ++r) {
        if (count[r + 1] == count[r]) continue;
        for (u32 i = count[r]; i < count[r + 1]; ++i) {
            if (i != count[r]) f << ',';
            f << name_of[order[i]];
        }
        f << '\n';
    }
    files.commit();
}

// the same into PREFIX_kSpider_clusters_<cutoff*100>%.tsv
void write_cluster_file(const std::string& prefix, const double threshold, const std::vector<u32>& label,
                        const std::vector<std::string>& name_of) {
    write_cluster_file_as(prefix + "_kSpider_clusters_" + py_float_repr(threshold) + "%.tsv", label, name_of);
}

// PREFIX.namesMap -> name of node index v = id - 1 (ks_clustering.py:56-61); ids must be 1..N
void read_names_map(const std::string& prefix, std::vector<std::string>& name_of) {
    std::unordered_map<long long, std::string> names;   // id -> name (a later row of the same id replaces the earlier)
    std::ifstream f(prefix + ".namesMap");
    if (!f) throw std::runtime_error("cannot open " + prefix + ".namesMap");
    std::string line;
    std::getline(f, line);   // the count line
    while (std::getline(f, line)) {
        const std::string s = strip(line);
        size_t sp = 0;
        while (sp < s.size() && !std::isspace((unsigned char)s[sp])) ++sp;
        size_t nb = sp;
        while (nb < s.size() && std::isspace((unsigned char)s[nb])) ++nb;
        size_t ne = nb;
        while (ne < s.size() && !std::isspace((unsigned char)s[ne])) ++ne;
        long long id;
        if (!parse_id(s.substr(0, sp), id) || ne == nb) throw std::runtime_error("malformed row in " + prefix + ".namesMap");
        names[id] = s.substr(nb, ne - nb);
    }
    const u64 N = names.size();
    if (N >= (1ull << 32)) throw std::runtime_error("more than 2^32 names");
    name_of.assign((size_t)N, std::string());
    for (u64 v = 1; v <= N; ++v) {
        auto it = names.find((long long)v);
        if (it == names.end()) throw std::runtime_error(".namesMap has no id " + std::to_string(v) + " (ids must be 1..N)");
        name_of[(size_t)v - 1] = it->second;
    }
}
}  // namespace ksp

extern "C" int ksp_components_edges(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                                    int dist_col, double cutoff, uint32_t* h_label) {
    if ((n_edges && (!d_edges || !d_kmer_counts)) || (n_nodes && !h_label)) { ksp::set_error("ksp_components_edges: NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { ksp::set_error("ksp_components_edges: dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_components_edges", device)) return rc;
    return ksp::cc_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoff, h_label, nullptr);
}

extern "C" int ksp_components_edges_ani(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                                        int ksize, double cutoff, uint32_t* h_label) {
    if ((n_edges && (!d_edges || !d_kmer_counts)) || (n_nodes && !h_label)) { ksp::set_error("ksp_components_edges_ani: NULL argument"); return KSP_E_ARG; }
    if (ksize < 1) { ksp::set_error("ksp_components_edges_ani: ksize < 1"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_components_edges_ani", device)) return rc;
    return ksp::cc_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, 6, cutoff, h_label, nullptr, ksize);
}

extern "C" int ksp_edges_ani(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int ksize, double* d_ani) {
    if (n_edges && (!d_edges || !d_kmer_counts || !d_ani)) { ksp::set_error("ksp_edges_ani: NULL argument"); return KSP_E_ARG; }
    if (ksize < 1) { ksp::set_error("ksp_edges_ani: ksize < 1"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_edges_ani", device)) return rc;
    if (n_edges == 0) return KSP_OK;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    double* d_table = nullptr;
    u32* d_nan = nullptr;
    u32 h_nan = 0;
    if ((rc = ksp::upload_ani_table(ksize, A, &d_table))) return rc;
    if ((rc = A.alloc(&d_nan, 1))) return rc;
    KSP_TRY_HIP(hipMemsetAsync(d_nan, 0, 4, nullptr));
    {   // a gather per edge: grid-stride over at most 8 workgroups per CU
        const unsigned g = (unsigned)std::min<u64>((n_edges + 255) / 256, 2048);
        hipLaunchKernelGGL(k_edges_ani, dim3(g), dim3(256), 0, nullptr, d_edges, n_edges, d_kmer_counts, d_table, d_ani, d_nan);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipMemcpy(&h_nan, d_nan, 4, hipMemcpyDeviceToHost));
        if (h_nan) { ksp::set_error("ksp_edges_ani: an edge has a NaN containment (0 shared k-mers of a source with 0 k-mers): it has no ANI"); rc = KSP_E_ARG; }
    }
done:
    return rc;
}

extern "C" int kspider_cluster(const char* index_prefix, const char* dist_type, double cutoff) {
    if (!index_prefix) { ksp::set_error("kspider_cluster: index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (!col) { ksp::set_error("kspider_cluster: unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)"); return KSP_E_ARG; }
    const double threshold = cutoff * 100.0;   // (ks_clustering.py: cutoff = float(cutoff) * 100)
    try {
        std::vector<std::string> name_of;
        std::vector<u32> ea, eb;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double d, const std::string&) {
            if (d < threshold) return;   // (a NaN is not below anything: kept, as in the reference)
            ksp::check_row_nodes(a, b, name_of.size());
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
        });
        const u64 N = name_of.size();
        std::vector<u32> label((size_t)N);
        const int rc = ksp_components(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), ea.size(), label.data());
        if (rc) return rc;
        ksp::write_cluster_file(prefix, threshold, label, name_of);
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_cluster: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_cluster: ") + e.what());
        return KSP_E_IO;
    }
}

namespace ksp {
// What both ladder calls leave on disk: one cluster file per distinct cut-off (write_cluster_file: the name and the bytes of
// kspider_cluster) and PREFIX_kSpider_cluster_sweep_<dist>.tsv, one row per distinct cut-off, ascending.  labels: n_cutoffs
// rows of name_of.size() node labels in the caller's order; kept[i] = the rows cut-off i keeps.  Cut-offs are distinct when
// the text of cutoff * 100 — the file name — is.  On a failure every file this call created is removed again.
void write_sweep_outputs(const std::string& prefix, const std::string& dist, const double* cutoffs, const uint32_t n_cutoffs, const uint32_t* labels,
                         const uint64_t* kept, const std::vector<std::string>& name_of) {
    const u64 N = name_of.size();
    std::vector<u32> pick;   // one caller index per distinct cut-off, ascending
    for (u32 i = 0; i < n_cutoffs; ++i) pick.push_back(i);
    std::stable_sort(pick.begin(), pick.end(), [&](const u32 x, const u32 y) { return cutoffs[x] * 100.0 < cutoffs[y] * 100.0; });
    pick.erase(std::unique(pick.begin(), pick.end(), [&](const u32 x, const u32 y) { return py_float_repr(cutoffs[x] * 100.0) == py_float_repr(cutoffs[y] * 100.0); }),
               pick.end());
    auto exists = [](const std::string& path) { return (bool)std::ifstream(path); };
    std::vector<std::string> created;
    const std::string summary = prefix + "_kSpider_cluster_sweep_" + dist + ".tsv";
    try {
        std::string rows = "cutoff_percent\tedges\tclusters\tsingletons\tlargest\n";
        for (const u32 i : pick) {
            const std::vector<u32> label(labels + (u64)i * N, labels + (u64)(i + 1) * N);
            const std::string text = py_float_repr(cutoffs[i] * 100.0), out = prefix + "_kSpider_clusters_" + text + "%.tsv";
            if (!exists(out)) created.push_back(out);
            write_cluster_file(prefix, cutoffs[i] * 100.0, label, name_of);
            std::vector<u32> size((size_t)N, 0);
            for (u64 v = 0; v < N; ++v) ++size[label[v]];
            u64 clusters = 0, singletons = 0, largest = 0;
            for (u64 v = 0; v < N; ++v) {
                clusters += size[v] != 0;
                singletons += size[v] == 1;
                largest = std::max<u64>(largest, size[v]);
            }
            rows += text + "\t" + std::to_string(kept[i]) + "\t" + std::to_string(clusters) + "\t" + std::to_string(singletons) + "\t" + std::to_string(largest) + "\n";
        }
        if (!exists(summary)) created.push_back(summary);
        write_file_atomically(summary, rows);
    } catch (...) {
        for (const std::string& path : created) std::remove(path.c_str());
        throw;
    }
}
}  // namespace ksp

extern "C" int kspider_cluster_sweep(const char* index_prefix, const char* dist_type, const double* cutoffs, uint32_t n_cutoffs) {
    if (!index_prefix) { ksp::set_error("kspider_cluster_sweep: index_prefix is NULL"); return KSP_E_ARG; }
    if (!cutoffs || n_cutoffs < 1 || n_cutoffs > KSP_SWEEP_MAX_CUTOFFS) {
        ksp::set_error("kspider_cluster_sweep: between 1 and " + std::to_string(KSP_SWEEP_MAX_CUTOFFS) + " cut-offs");
        return KSP_E_ARG;
    }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (!col) { ksp::set_error("kspider_cluster_sweep: unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)"); return KSP_E_ARG; }
    const u32 K = n_cutoffs;
    for (u32 i = 0; i < K; ++i)
        if (cutoffs[i] != cutoffs[i]) { ksp::set_error("kspider_cluster_sweep: a cut-off is NaN"); return KSP_E_ARG; }
    // The row test of kspider_cluster is `value * 100 < cutoff * 100 -> dropped`, in double: the rows a cut-off keeps shrink
    // as cutoff * 100 grows, so the rank of a cut-off is its place among the thresholds, ascending, and a row's level is the
    // number of thresholds it is not below (a NaN: all of them).
    std::vector<u32> caller_of(K);   // rank -> caller's index
    for (u32 i = 0; i < K; ++i) caller_of[i] = i;
    std::stable_sort(caller_of.begin(), caller_of.end(), [&](const u32 x, const u32 y) { return cutoffs[x] * 100.0 < cutoffs[y] * 100.0; });
    std::vector<double> threshold(K);
    for (u32 r = 0; r < K; ++r) threshold[r] = cutoffs[caller_of[r]] * 100.0;
    try {
        std::vector<std::string> name_of;
        std::vector<u32> ea, eb;
        std::vector<uint8_t> level;
        std::vector<u64> per_level((size_t)K + 1, 0);
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double d, const std::string&) {
            // the thresholds ascend: the level is the place of the first one the row is below (a NaN is below none)
            const u32 l = d != d ? K : (u32)(std::upper_bound(threshold.begin(), threshold.end(), d) - threshold.begin());
            ++per_level[l];
            if (!l) return;
            ksp::check_row_nodes(a, b, name_of.size());
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            level.push_back((uint8_t)l);
        });
        const u64 N = name_of.size();
        std::vector<u32> by_rank((size_t)K * N), labels((size_t)K * N);
        const int rc = ksp_components_sweep(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), level.data(), ea.size(), K, by_rank.data());
        if (rc) return rc;
        std::vector<u64> kept(K);
        u64 above = 0;
        for (u32 r = K; r-- > 0;) {
            above += per_level[r + 1];
            kept[caller_of[r]] = above;   // the rows of level > r
            std::copy(by_rank.begin() + (size_t)r * N, by_rank.begin() + (size_t)(r + 1) * N, labels.begin() + (size_t)caller_of[r] * N);
        }
        ksp::write_sweep_outputs(prefix, dt, cutoffs, K, labels.data(), kept.data(), name_of);
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_cluster_sweep: out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_cluster_sweep: ") + e.what());
        return KSP_E_IO;
    }
}
