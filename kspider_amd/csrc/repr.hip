// kspider_repr_sketches(): the reference's `repr_sketches` tool — apps/repr_sketches.cpp:27-33,38-43 — with the
// neighbour counts and their ranking computed on the GPU, from a pairwise TSV or straight from the join's edge records.
//
// What the reference does (restated, nothing copied):
//   * for every data line of PREFIX_kSpider_pairwise.tsv (header skipped): containment = stof(column 4), a float; the row
//     passes when containment > 0.20 — the float promoted to double against the double literal, strictly (:27-33);
//   * a passing row adds 1 to the count of stoi(column 0) and of stoi(column 1);
//   * the ids with a count are sorted by count, largest first, and printed as "id: count" lines (:38-43).
// Deliberate difference: the order among equal counts is whatever an unstable std::sort makes of the hash map's
// iteration order there; here it is canonical — count descending, then id ascending.
//
// Column 4 is the 6-significant-digit text of a float (src/pairwise.cpp:266-273), so the test on an edge record is NOT
// `v > 0.2` on the float: 0.1999996 prints "0.2", which stof reads as 0.2f = 0.200000003 > 0.20.  Printing and parsing are
// monotone, so the rows that pass are exactly those whose float is not below ONE critical float (ksp::repr_critical,
// found by bisection with the text test itself as the predicate); the device compares against that.
//
// Device side: one pass over the records adds 1 to a u32 counter of both ends of every kept edge.  Up to kDegreeLdsNodes
// nodes the counters are private to the workgroup in LDS and flushed with one global atomic per non-zero counter; above,
// they are global atomics.  Either way the lanes of a wave that hold the same node in a row are combined first: the join
// delivers edges sorted by (source_1, source_2), so 64 consecutive lanes usually share source_1 (and a star shares its
// centre everywhere) — one atomic per run instead of 64 on one address.
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

// Counters in LDS up to this many nodes.  A CU has 160 KiB of LDS and 32 wave slots; a workgroup of kDegreeThreads = 1024
// threads is 16 waves, so two resident workgroups fill the CU, and each may then hold at most 80 KiB: 16 384 u32 counters
// are 64 KiB, the largest power of two that keeps both resident.
constexpr u32 kDegreeLdsNodes = 16384;
constexpr int kDegreeThreads = 1024;
constexpr u32 kDegreeEdgesPerGroup = 16384;   // at least this many edges per workgroup of the LDS path: the zeroing and the flush cost n_nodes each
constexpr u32 kNoNode = 0xFFFFFFFFu;          // (never a node: nodes are < n_nodes <= 2^32 - 1)

// Every lane of the wave calls this with the node it adds 1 to (kNoNode: none).  A run of consecutive lanes with the same
// node becomes one add of the run's length by its first lane.
__device__ inline void wave_add_runs(u32* __restrict__ counters, const u32 node, const u32 lane) {
    const u32 prev = __shfl_up(node, 1);   // (lane 0 reads its own value)
    const bool head = lane == 0 || node != prev;
    const unsigned long long heads = __ballot(head);
    if (head && node != kNoNode) {
        const unsigned long long above = (heads >> lane) >> 1;   // heads of the lanes after mine
        const u32 len = above ? (u32)__ffsll((long long)above) : 64u - lane;
        atomicAdd(&counters[node], len);
    }
}

// kRecords: the join's edge records, cut by the critical float (NaN never passes); an edge naming a node >= n_nodes is the
// caller's error and is not counted.  !kRecords: plain (a[], b[]) node arrays, every pair counted (the TSV form: the host
// applied the text test).  The loop bound is uniform over the wave (base is a multiple of 64): every lane takes part in
// the shuffle and the ballot of wave_add_runs.
template <bool kLds, bool kRecords>
__global__ __launch_bounds__(kDegreeThreads) void k_degree(const ksp_edge* __restrict__ ed, const u32* __restrict__ a, const u32* __restrict__ b,
                                                           const u64 m, const u32 n_nodes, const u32* __restrict__ cnt, const int col,
                                                           const float vcrit, u32* __restrict__ degree) {
    extern __shared__ u32 lds_degree[];
    if (kLds) {
        for (u32 v = threadIdx.x; v < n_nodes; v += blockDim.x) lds_degree[v] = 0;
        __syncthreads();
    }
    const u32 lane = threadIdx.x & 63;
    for (u64 base = (u64)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < m; base += (u64)gridDim.x * blockDim.x) {
        const u64 e = base + lane;
        u32 na = kNoNode, nb = kNoNode;
        if (e < m) {
            if (kRecords) {
                const ksp_edge x = ed[e];
                if (x.source_1 < n_nodes && x.source_2 < n_nodes) {
                    const float v = edge_col_value(x, cnt, col);
                    if (!(v < vcrit) && v == v) { na = x.source_1; nb = x.source_2; }
                }
            } else {
                const u32 s = a[e], t = b[e];
                if (s < n_nodes && t < n_nodes) { na = s; nb = t; }
            }
        }
        if (kLds) {
            wave_add_runs(lds_degree, na, lane);
            wave_add_runs(lds_degree, nb, lane);
        } else {
            wave_add_runs(degree, na, lane);
            wave_add_runs(degree, nb, lane);
        }
    }
    if (kLds) {
        __syncthreads();
        for (u32 v = threadIdx.x; v < n_nodes; v += blockDim.x) {
            const u32 c = lds_degree[v];
            if (c) atomicAdd(&degree[v], c);
        }
    }
}

// one sortable key per node: ascending order of (~count << 32 | node) is (count descending, node ascending)
__global__ void k_degree_keys(const u32* __restrict__ degree, const u32 n_nodes, u64* __restrict__ keys) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n_nodes) keys[v] = ((u64)(~degree[v]) << 32) | v;
}
struct HasNeighbour {
    __host__ __device__ bool operator()(const u64& key) const { return (key >> 32) != 0xFFFFFFFFull; }   // (count != 0)
};

template <bool kRecords>
int launch_degree(const ksp_edge* d_edges, const u32* d_a, const u32* d_b, const u64 m, const u32 n_nodes, const u32* d_cnt, const int col,
                  const float vcrit, u32* d_degree) {
    int rc = KSP_OK;
    int device = 0, cus = 0;
    const char* lds_env = std::getenv("KSP_DEGREE_LDS");   // "0": global counters at every size (tests)
    const bool use_lds = n_nodes <= kDegreeLdsNodes && !(lds_env && std::strcmp(lds_env, "0") == 0);
    KSP_TRY_HIP(hipGetDevice(&device));
    KSP_TRY_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    if (cus < 1) cus = 1;
    if (use_lds) {
        const size_t lds = (size_t)n_nodes * sizeof(u32);
        const unsigned grid = (unsigned)std::min<u64>((m + kDegreeEdgesPerGroup - 1) / kDegreeEdgesPerGroup, 2ull * (u64)cus);
        KSP_TRY_HIP(hipFuncSetAttribute((const void*)k_degree<true, kRecords>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_degree<true, kRecords>), dim3(grid), dim3(kDegreeThreads), lds, nullptr, d_edges, d_a, d_b, m, n_nodes, d_cnt, col, vcrit, d_degree);
    } else {
        const unsigned grid = (unsigned)std::min<u64>((m + kDegreeThreads - 1) / kDegreeThreads, 2ull * (u64)cus);
        hipLaunchKernelGGL((k_degree<false, kRecords>), dim3(grid), dim3(kDegreeThreads), 0, nullptr, d_edges, d_a, d_b, m, n_nodes, d_cnt, col, vcrit, d_degree);
    }
    KSP_TRY_HIP(hipGetLastError());
done:
    return rc;
}

// The counts of n_edges > 0 edges over n_nodes > 0 nodes on the CURRENT device — records cut by vcrit, or (d_a, d_b) pairs —
// and, when h_node is given, the nodes with a count in (count descending, node ascending) order.
int degrees_on_device(const u32 n_nodes, const ksp_edge* d_edges, const u32* d_a, const u32* d_b, const u64 n_edges, const u32* d_cnt, const int col,
                      const float vcrit, u32* h_degree, u32* h_node, u32* h_count, u32* n_ranked) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32* d_degree = nullptr;
    u64 *d_keys = nullptr, *d_sel = nullptr, *d_sorted = nullptr;
    unsigned long long* d_nsel = nullptr;
    void* d_tmp = nullptr;
    if ((rc = A.alloc(&d_degree, (size_t)n_nodes))) goto done;
    KSP_TRY_HIP(hipMemsetAsync(d_degree, 0, (size_t)n_nodes * 4, nullptr));
    if (d_edges) rc = launch_degree<true>(d_edges, nullptr, nullptr, n_edges, n_nodes, d_cnt, col, vcrit, d_degree);
    else rc = launch_degree<false>(nullptr, d_a, d_b, n_edges, n_nodes, nullptr, 0, 0.0f, d_degree);
    if (rc) goto done;
    if (h_degree) KSP_TRY_HIP(hipMemcpy(h_degree, d_degree, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    if (h_node) {
        unsigned long long nsel = 0;
        size_t tb = 0;
        *n_ranked = 0;
        if ((rc = A.alloc(&d_keys, (size_t)n_nodes)) || (rc = A.alloc(&d_sel, (size_t)n_nodes)) || (rc = A.alloc(&d_nsel, 1))) goto done;
        hipLaunchKernelGGL(k_degree_keys, dim3((unsigned)(((u64)n_nodes + 255) / 256)), dim3(256), 0, nullptr, d_degree, n_nodes, d_keys);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(rocprim::select(nullptr, tb, d_keys, d_sel, d_nsel, (size_t)n_nodes, HasNeighbour(), (hipStream_t) nullptr));
        if ((rc = A.alloc_bytes(&d_tmp, tb ? tb : 8))) goto done;
        KSP_TRY_HIP(rocprim::select(d_tmp, tb, d_keys, d_sel, d_nsel, (size_t)n_nodes, HasNeighbour(), (hipStream_t) nullptr));
        KSP_TRY_HIP(hipMemcpy(&nsel, d_nsel, 8, hipMemcpyDeviceToHost));
        (void)A.release(d_tmp);   // (the select's scratch goes before the sort's comes: the peak stays the larger of the two)
        if (nsel) {
            std::vector<u64> keys((size_t)nsel);
            if ((rc = A.alloc(&d_sorted, (size_t)nsel))) goto done;
            KSP_TRY_HIP(rocprim::radix_sort_keys(nullptr, tb, d_sel, d_sorted, (size_t)nsel, 0, 64, (hipStream_t) nullptr));
            if ((rc = A.alloc_bytes(&d_tmp, tb ? tb : 8))) goto done;
            KSP_TRY_HIP(rocprim::radix_sort_keys(d_tmp, tb, d_sel, d_sorted, (size_t)nsel, 0, 64, (hipStream_t) nullptr));
            KSP_TRY_HIP(hipMemcpy(keys.data(), d_sorted, (size_t)nsel * 8, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < keys.size(); ++i) {
                h_node[i] = (u32)keys[i];
                h_count[i] = ~(u32)(keys[i] >> 32);
            }
        }
        *n_ranked = (u32)nsel;
    }
done:
    return rc;
}

int check_edges_args(const char* who, const ksp_edge* d_edges, const u64 n_edges, const u32* d_kmer_counts, const int dist_col, const double threshold) {
    if (n_edges && (!d_edges || !d_kmer_counts)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error(std::string(who) + ": the threshold is NaN"); return KSP_E_ARG; }
    if (n_edges >= (1ull << 32)) { ksp::set_error(std::string(who) + ": 2^32 edges or more (the neighbour counters are 32-bit)"); return KSP_E_LIMIT; }
    return KSP_OK;
}

int dist_column(const char* who, const char* dist_type, int* col) {
    const std::string dt = dist_type && *dist_type ? dist_type : "avg_cont";
    if (dt == "min_cont") *col = 3;
    else if (dt == "avg_cont") *col = 4;
    else if (dt == "max_cont") *col = 5;
    else {
        ksp::set_error(std::string(who) + ": distance '" + dt + "' is not min_cont, avg_cont or max_cont" +
                       (dt == "ani" ? " (the reference tool reads a containment column of the pairwise TSV; the ANI column is a separate file)" : ""));
        return KSP_E_ARG;
    }
    return KSP_OK;
}

std::string strip(const std::string& s) {
    size_t b = 0, e = s.size();
    while (b < e && std::isspace((unsigned char)s[b])) ++b;
    while (e > b && std::isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}

struct RowError {   // a row the parsers refuse: the status and a message that names the line
    int rc;
    std::string msg;
};

}  // namespace

namespace ksp {
bool repr_text_passes(const float v, const double threshold) {
    char buf[64];
    const int n = ksp_format_float(v, buf);
    buf[n] = 0;
    const float back = std::strtof(buf, nullptr);
    return (double)back > threshold;
}

// Bisection over the non-negative floats (their bit patterns are ordered as the values are) for the smallest one that passes.
void repr_critical(const double threshold, float* vcrit, int* none_pass) {
    auto passes = [&](const uint32_t bits) {
        float v;
        std::memcpy(&v, &bits, 4);
        return repr_text_passes(v, threshold);
    };
    const uint32_t inf_bits = 0x7F800000u;
    *none_pass = 0;
    *vcrit = 0;
    if (!passes(inf_bits)) { *none_pass = 1; return; }
    uint32_t lo = 0, hi = inf_bits;   // the smallest pattern that passes lies in [lo, hi]; hi passes
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (passes(mid)) hi = mid; else lo = mid + 1;
    }
    std::memcpy(vcrit, &hi, 4);
}

int repr_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col,
                         const double threshold, uint32_t* h_degree, uint32_t* h_node, uint32_t* h_count, uint32_t* n_ranked) {
    float vcrit = 0;
    int none_pass = 0;
    repr_critical(threshold, &vcrit, &none_pass);
    if (h_degree && n_nodes) std::memset(h_degree, 0, (size_t)n_nodes * 4);
    if (n_ranked) *n_ranked = 0;
    if (n_edges == 0 || n_nodes == 0 || none_pass) return KSP_OK;   // nothing can be counted: no kernel runs
    return degrees_on_device(n_nodes, d_edges, nullptr, nullptr, n_edges, d_cnt, col, vcrit, h_degree, h_node, h_count, n_ranked);
}

// (derep.hip) the counting kernel and the key kernel on the caller's buffers of the CURRENT device, nothing read back: d_degree
// (n_nodes counters, zeroed here) and d_keys, the key of EVERY node, not only of those with a neighbour.  Records cut by vcrit
// (d_edges) or (d_a, d_b) pairs, as in degrees_on_device.
int degree_keys_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint32_t* d_a, const uint32_t* d_b, const uint64_t n_edges,
                          const uint32_t* d_cnt, const int col, const float vcrit, uint32_t* d_degree, uint64_t* d_keys) {
    int rc = KSP_OK;
    KSP_TRY_HIP(hipMemsetAsync(d_degree, 0, (size_t)n_nodes * 4, nullptr));
    if (d_edges) rc = launch_degree<true>(d_edges, nullptr, nullptr, n_edges, n_nodes, d_cnt, col, vcrit, d_degree);
    else rc = launch_degree<false>(nullptr, d_a, d_b, n_edges, n_nodes, nullptr, 0, 0.0f, d_degree);
    if (rc) goto done;
    hipLaunchKernelGGL(k_degree_keys, dim3((unsigned)(((u64)n_nodes + 255) / 256)), dim3(256), 0, nullptr, (const u32*)d_degree, n_nodes, (u64*)d_keys);
    KSP_TRY_HIP(hipGetLastError());
done:
    return rc;
}

void write_repr_file(const std::string& out_path, const std::vector<uint32_t>& ids, const uint32_t* node, const uint32_t* count, const uint64_t n_ranked) {
    std::string text;
    text.reserve((size_t)n_ranked * 16);
    for (u64 i = 0; i < n_ranked; ++i) {
        text += std::to_string(ids[node[i]]);
        text += ": ";
        text += std::to_string(count[i]);
        text += '\n';
    }
    if (out_path.empty()) {
        if (std::fwrite(text.data(), 1, text.size(), stdout) != text.size() || std::fflush(stdout) != 0) throw std::runtime_error("write error on stdout");
        return;
    }
    write_file_atomically(out_path, text);
}
}  // namespace ksp

extern "C" int ksp_repr_critical(double threshold, float* vcrit, int* none_pass) {
    if (!vcrit || !none_pass) { ksp::set_error("ksp_repr_critical: NULL argument"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error("ksp_repr_critical: the threshold is NaN"); return KSP_E_ARG; }
    ksp::repr_critical(threshold, vcrit, none_pass);
    return KSP_OK;
}

extern "C" int ksp_edges_degrees(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                                 int dist_col, double threshold, uint32_t* h_degree) {
    if (const int rc = check_edges_args("ksp_edges_degrees", d_edges, n_edges, d_kmer_counts, dist_col, threshold)) return rc;
    if (n_nodes && !h_degree) { ksp::set_error("ksp_edges_degrees: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_edges_degrees", device)) return rc;
    return ksp::repr_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, threshold, h_degree, nullptr, nullptr, nullptr);
}

extern "C" int ksp_edges_repr(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                              int dist_col, double threshold, uint32_t* h_node, uint32_t* h_count, uint32_t* n_ranked) {
    if (const int rc = check_edges_args("ksp_edges_repr", d_edges, n_edges, d_kmer_counts, dist_col, threshold)) return rc;
    if (!n_ranked || (n_nodes && (!h_node || !h_count))) { ksp::set_error("ksp_edges_repr: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_edges_repr", device)) return rc;
    return ksp::repr_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, threshold, nullptr, h_node, h_count, n_ranked);
}

extern "C" int kspider_repr_sketches(const char* pairwise_tsv, const char* dist_type, double threshold, const char* out_path) {
    if (!pairwise_tsv) { ksp::set_error("kspider_repr_sketches: pairwise_tsv is NULL"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error("kspider_repr_sketches: the threshold is NaN"); return KSP_E_ARG; }
    int col = 4;
    if (const int rc = dist_column("kspider_repr_sketches", dist_type, &col)) return rc;
    const std::string path = pairwise_tsv;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr;
    try {
        // the rows that pass the text test, as the reference reads them: columns 0 and 1 and the chosen column
        std::vector<u32> ea, eb;
        {
            std::ifstream f(path);
            if (!f) throw std::runtime_error("cannot open " + path);
            std::string line;
            std::getline(f, line);   // header
            u64 lineno = 1;
            while (std::getline(f, line)) {
                ++lineno;
                const std::string where = path + " line " + std::to_string(lineno);
                size_t begin[6], end[6];
                int ncol = 0;
                for (size_t b = 0; ncol < 6; ++ncol) {
                    const size_t e = line.find('\t', b);
                    begin[ncol] = b;
                    end[ncol] = e == std::string::npos ? line.size() : e;
                    if (e == std::string::npos) { ++ncol; break; }
                    b = e + 1;
                }
                if (ncol <= col) throw RowError{KSP_E_IO, where + ": " + std::to_string(ncol) + " columns, the distance is column " + std::to_string(col)};
                long long id[2];
                for (int c = 0; c < 2; ++c) {   // the reference's stoi: a decimal integer that fits an int
                    const std::string t = strip(line.substr(begin[c], end[c] - begin[c]));
                    char* stop = nullptr;
                    errno = 0;
                    id[c] = std::strtoll(t.c_str(), &stop, 10);
                    if (t.empty() || errno == EINVAL || !stop || *stop) throw RowError{KSP_E_IO, where + ": '" + t + "' is not an id"};
                    if (errno == ERANGE || id[c] < 0 || id[c] > 2147483647ll) throw RowError{KSP_E_ARG, where + ": id " + t + " is not in [0, 2^31 - 1]"};
                }
                const std::string t = strip(line.substr(begin[col], end[col] - begin[col]));
                char* stop = nullptr;
                const float v = std::strtof(t.c_str(), &stop);   // the reference's stof
                if (t.empty() || !stop || *stop) throw RowError{KSP_E_IO, where + ": '" + t + "' is not a number"};
                if (!((double)v > threshold)) continue;
                if (ea.size() >= 0xFFFFFFFFull) throw RowError{KSP_E_LIMIT, "2^32 rows or more pass (the neighbour counters are 32-bit)"};
                ea.push_back((u32)id[0]);
                eb.push_back((u32)id[1]);
            }
            if (f.bad()) throw std::runtime_error("read error on " + path);
        }
        // dense node = rank of the id among the ids that pass: node order is id order
        std::vector<u32> ids(ea);
        ids.insert(ids.end(), eb.begin(), eb.end());
        std::sort(ids.begin(), ids.end());
        ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
        for (auto* arr : {&ea, &eb})
            for (u32& x : *arr) x = (u32)(std::lower_bound(ids.begin(), ids.end(), x) - ids.begin());
        const u32 N = (u32)ids.size();
        const u64 M = ea.size();
        std::vector<u32> node((size_t)N), count((size_t)N);
        u32 n_ranked = 0;
        if ((rc = ksp::set_device("kspider_repr_sketches", ksp::device_from_env()))) return rc;
        if (M) {
            if ((rc = ksp::upload_pairs(A, ea.data(), eb.data(), M, &d_a, &d_b))) return rc;
            if ((rc = degrees_on_device(N, nullptr, d_a, d_b, M, nullptr, 0, 0.0f, nullptr, node.data(), count.data(), &n_ranked))) return rc;
        }
        ksp::write_repr_file(out_path && *out_path ? out_path : "", ids, node.data(), count.data(), n_ranked);
    } catch (const RowError& e) {
        ksp::set_error("kspider_repr_sketches: " + e.msg);
        rc = e.rc;
    } catch (const std::bad_alloc&) {
        ksp::set_error("kspider_repr_sketches: out of host memory");
        rc = KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string("kspider_repr_sketches: ") + e.what());
        rc = KSP_E_IO;
    }
    return rc;
}
