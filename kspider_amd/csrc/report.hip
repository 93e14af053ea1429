// The cluster report: for every connected component of the kept records its size, edge count, value range, the
// medoid (the member of the largest strength) and how many members the medoid touches, and for every node its label, degree,
// strength and the record that links it to its medoid — taken from the join's edge records while they are in HBM, or from host
// edges the caller has cut.  The definitions are in include/kspider_amd.h.
//
//   labels      cluster.hip's hooking and pointer jumping (cc_rounds_on_device), strict: a record naming a node >= n_nodes and a
//               self pair are skipped before anything is read through them.  The labels stay in device memory.
//   accumulate  k_report_accumulate: one pass over the records in chunks of KSP_REPORT_CHUNK_EDGES per 256-thread workgroup.  All
//               atomics are integer: 64-bit adds of q = floor(v * 2^32) and of counts, atomicMin / atomicMax on the bit pattern of
//               the value (no value is negative, so the patterns order as the floats do).  Most records of a real run belong to
//               ONE giant component, and the join's records are sorted by (source_1, source_2), so everything that shares an
//               address is summed on chip first:
//                 source_1 side   the consecutive lanes of a wave that hold the same source_1 make one run: a segmented scan
//                                 over the 64 lanes sums degree and q, the run's last lane issues one set of atomics
//                 cluster side    when every kept record of the chunk carries one label: a reduction over the workgroup through
//                                 LDS and one set of atomics for the chunk; otherwise one set per run of equal label per wave
//                 source_2 side   one atomic per record: those addresses are spread
//               The same pass finds a kept value outside [0, 1] and sets one flag word; the host refuses.
//   medoid      two passes over the nodes: atomicMax of the strength into the root's slot, atomicMin of the node among those
//               that equal it (a 96-bit (strength, node) key does not fit one atomic)
//   links       one more pass over the records: a kept record with one end equal to its cluster's medoid lowers via[other end]
//               to its index (atomicMin)
//   rows        sizes, covered and the compaction of the by-root slots into rows in root order are made by the HOST from the
//               arrays it copies back (64 bytes per node): one pass over n_nodes, nothing the device would do better
// Every wave helper below is called by all 64 lanes (the loads are padded with records that are not kept, no lane leaves the
// loop early); no workgroup ever waits on another; every loop is bounded by a size the host computed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "cluster_inputs.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef unsigned long long ull;

static_assert(sizeof(ksp_cluster_row) == 48 && sizeof(ksp_member_row) == 24, "the layouts of the header");

namespace {

constexpr u32 kChunk = KSP_REPORT_CHUNK_EDGES;   // (the reasons for 2 048 records per 256 threads: cut.hip; not measured here)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = (int)(kChunk / kThreads);   // records per lane and chunk
constexpr u32 kNone = 0xFFFFFFFFu;
static_assert(kIters * kThreads == (int)kChunk, "a chunk is whole ballots of every wave");

thread_local ksp::ReportTrace g_trace;   // (ksp_debug_report_counts)

// the edges of one call: the join's records cut on the device (ed, cnt, col, vcrit, mode) or valued pairs, all kept (a, b, val)
struct ReportIn {
    const ksp_edge* ed = nullptr;
    const u32* cnt = nullptr;
    int col = 0, mode = 0;
    float vcrit = 0;
    const u32 *a = nullptr, *b = nullptr;
    const float* val = nullptr;
};

// the device memory of one report
struct ReportArrays {
    u32 *label = nullptr, *deg = nullptr, *via = nullptr, *c_min = nullptr, *c_max = nullptr, *medoid = nullptr, *words = nullptr;
    ull *strength = nullptr, *c_edges = nullptr, *c_nan = nullptr, *c_sumq = nullptr, *best = nullptr, *counts = nullptr;
};

// Record e of the call: its ends, its value and whether it is kept; e >= n is a record that is not kept (the padding of a
// wave's last ballot).  Nothing is read through an end that is no node.
template <bool kRecords>
__device__ inline void report_record(const ReportIn& in, const u64 n, const u32 N, const u64 e, u32& s, u32& t, float& v, bool& kept) {
    s = t = kNone;
    v = 0;
    kept = false;
    if (e >= n) return;
    if (kRecords) {
        const ksp_edge x = in.ed[e];
        s = x.source_1; t = x.source_2;
        if (s >= N || t >= N || s == t) return;
        v = edge_col_value(x, in.cnt, in.col);
        kept = in.mode ? v != v : !(v < in.vcrit);   // (cc_edge_kept on the value at hand)
    } else {
        s = in.a[e]; t = in.b[e];
        if (s >= N || t >= N || s == t) return;
        v = in.val[e];
        if (v == 0) v = 0;   // (-0 is 0: the bit patterns have to order as the values do)
        kept = true;
    }
}
// q of a kept value inside the domain; 0 for a NaN (it has no q) and for a value the call is refused for
__device__ inline u64 report_q(const float v) { return v >= 0 && v <= 1 ? (u64)((double)v * 4294967296.0) : 0; }

__device__ inline u64 shfl_up64(const u64 x, const int d) {
    const u32 lo = (u32)__shfl_up((int)(u32)x, d), hi = (u32)__shfl_up((int)(u32)(x >> 32), d);
    return ((u64)hi << 32) | lo;
}
__device__ inline u64 shfl_xor64(const u64 x, const int m) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, m), hi = (u32)__shfl_xor((int)(u32)(x >> 32), m);
    return ((u64)hi << 32) | lo;
}
// The run of consecutive lanes that hold my key: [start, end).  Every lane of the wave calls it.
__device__ inline void wave_run(const u32 key, const u32 lane, u32& start, u32& end) {
    const u32 prev = (u32)__shfl_up((int)key, 1);
    const ull heads = __ballot(lane == 0 || prev != key);
    start = 63u - (u32)__clzll((long long)(heads & (~0ull >> (63 - lane))));
    const ull after = lane == 63 ? 0ull : heads >> (lane + 1);
    end = after ? lane + (u32)__ffsll(after) : 64u;
}
__device__ inline ull run_mask(const u32 start, const u32 end) { return (end == 64 ? ~0ull : (1ull << end) - 1) & ~((1ull << start) - 1); }
// Inclusive scans inside the runs: lane l ends with op over the lanes start .. l of its run, so a run's last lane holds the
// run's total.  Six shuffle steps; every lane of the wave takes every step, the combine alone is conditional.
__device__ inline u64 run_scan_add(u64 x, const u32 start, const u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = shfl_up64(x, d);
        if (lane >= start + (u32)d) x += o;
    }
    return x;
}
__device__ inline u32 run_scan_min(u32 x, const u32 start, const u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)x, d);
        if (lane >= start + (u32)d && o < x) x = o;
    }
    return x;
}
__device__ inline u32 run_scan_max(u32 x, const u32 start, const u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)x, d);
        if (lane >= start + (u32)d && o > x) x = o;
    }
    return x;
}

// one set of cluster atomics: `edges` kept records of cluster `root`, `nans` of them NaN, the others summing to q in [mn, mx]
__device__ inline void cluster_add(const ReportArrays& R, const u32 root, const u64 edges, const u64 nans, const u64 q, const u32 mn, const u32 mx) {
    atomicAdd(&R.c_edges[root], (ull)edges);
    if (nans) atomicAdd(&R.c_nan[root], (ull)nans);
    if (q) atomicAdd(&R.c_sumq[root], (ull)q);
    if (edges > nans) {
        atomicMin(&R.c_min[root], mn);
        atomicMax(&R.c_max[root], mx);
    }
}

// R.words[0] = 1 when a kept value lies outside [0, 1]; R.counts[0 .. 3] += the trace of this workgroup, one add each at its end
template <bool kRecords>
__global__ __launch_bounds__(kThreads) void k_report_accumulate(const ReportIn in, const u64 n, const u64 n_chunks, const u32 N, const ReportArrays R) {
    __shared__ u32 sh_lo[2][kWaves], sh_hi[2][kWaves], sh_mm[kWaves][2];
    __shared__ ull sh_sum[kWaves][3], sh_trace[kWaves][3];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    ull w_kept = 0, w_node_sets = 0, w_cluster_sets = 0;   // of this wave: every lane holds the same numbers
    ull g_single = 0;                                      // of this workgroup: every thread holds the same number
    bool bad = false;
    u32 parity = 0;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x, parity ^= 1) {
        const u64 base = chunk * kChunk + (u64)wave * (kIters * 64);   // wave w owns the records [w * 512, (w + 1) * 512) of its chunk
        u32 s[kIters], t[kIters], L[kIters];
        float v[kIters];
        bool k[kIters];
#pragma unroll
        for (int i = 0; i < kIters; ++i) report_record<kRecords>(in, n, N, base + (u64)i * 64 + lane, s[i], t[i], v[i], k[i]);
        u32 lo = kNone, hi = 0;   // the smallest and the largest label among my kept records
#pragma unroll
        for (int i = 0; i < kIters; ++i) {
            L[i] = k[i] ? R.label[s[i]] : kNone;
            if (k[i]) { lo = L[i] < lo ? L[i] : lo; hi = L[i] > hi ? L[i] : hi; }
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) {
            const u32 ol = (u32)__shfl_xor((int)lo, m), oh = (u32)__shfl_xor((int)hi, m);
            lo = ol < lo ? ol : lo;
            hi = oh > hi ? oh : hi;
        }
        if (lane == 0) { sh_lo[parity][wave] = lo; sh_hi[parity][wave] = hi; }
        // ---- the node sides, while the labels of the other waves arrive
        u64 tq = 0;                 // my kept records: the sum of q, the NaN ones, all of them, the value range
        u32 tn = 0, te = 0, tmn = kNone, tmx = 0;
#pragma unroll
        for (int i = 0; i < kIters; ++i) {
            const bool nan = v[i] != v[i];
            if (k[i] && !nan && !(v[i] >= 0 && v[i] <= 1)) bad = true;
            const u64 q = k[i] ? report_q(v[i]) : 0;
            const u32 key = k[i] ? s[i] : kNone;
            u32 start, end;
            wave_run(key, lane, start, end);
            const u64 run_q = run_scan_add(q, start, lane);
            const bool tail = key != kNone && lane + 1 == end;
            if (tail) {
                atomicAdd(&R.deg[key], end - start);
                if (run_q) atomicAdd(&R.strength[key], (ull)run_q);
            }
            w_node_sets += (ull)__popcll(__ballot(tail));
            w_kept += (ull)__popcll(__ballot(k[i]));
            if (k[i]) {
                atomicAdd(&R.deg[t[i]], 1u);
                if (q) atomicAdd(&R.strength[t[i]], (ull)q);
                ++te;
                if (nan) ++tn;
                else {
                    const u32 bits = __float_as_uint(v[i]);
                    tq += q;
                    tmn = bits < tmn ? bits : tmn;
                    tmx = bits > tmx ? bits : tmx;
                }
            }
        }
        __syncthreads();
        lo = sh_lo[parity][0]; hi = sh_hi[parity][0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            lo = sh_lo[parity][w] < lo ? sh_lo[parity][w] : lo;
            hi = sh_hi[parity][w] > hi ? sh_hi[parity][w] : hi;
        }
        if (lo == kNone) continue;   // no kept record in the chunk (uniform over the workgroup)
        if (lo == hi) {
            // ---- one label: the chunk's sums through LDS, one set of atomics
            u64 te64 = te, tn64 = tn;
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                te64 += shfl_xor64(te64, m);
                tn64 += shfl_xor64(tn64, m);
                tq += shfl_xor64(tq, m);
                const u32 on = (u32)__shfl_xor((int)tmn, m), ox = (u32)__shfl_xor((int)tmx, m);
                tmn = on < tmn ? on : tmn;
                tmx = ox > tmx ? ox : tmx;
            }
            if (lane == 0) { sh_sum[wave][0] = te64; sh_sum[wave][1] = tn64; sh_sum[wave][2] = tq; sh_mm[wave][0] = tmn; sh_mm[wave][1] = tmx; }
            __syncthreads();
            if (threadIdx.x == 0) {
                u64 e = 0, nn = 0, q = 0;
                u32 mn = kNone, mx = 0;
                for (int w = 0; w < kWaves; ++w) {
                    e += sh_sum[w][0]; nn += sh_sum[w][1]; q += sh_sum[w][2];
                    mn = sh_mm[w][0] < mn ? sh_mm[w][0] : mn;
                    mx = sh_mm[w][1] > mx ? sh_mm[w][1] : mx;
                }
                cluster_add(R, lo, e, nn, q, mn, mx);
            }
            ++g_single;
        } else {
            // ---- several labels: one set of atomics per run of equal label per wave
#pragma unroll
            for (int i = 0; i < kIters; ++i) {
                const bool nan = v[i] != v[i];
                const u32 bits = __float_as_uint(v[i]);
                u32 start, end;
                wave_run(L[i], lane, start, end);
                const u64 run_q = run_scan_add(k[i] ? report_q(v[i]) : 0, start, lane);
                const u32 run_mn = run_scan_min(k[i] && !nan ? bits : kNone, start, lane);
                const u32 run_mx = run_scan_max(k[i] && !nan ? bits : 0u, start, lane);
                const ull nans = __ballot(k[i] && nan) & run_mask(start, end);
                const bool tail = L[i] != kNone && lane + 1 == end;
                if (tail) cluster_add(R, L[i], end - start, (u64)__popcll(nans), run_q, run_mn, run_mx);
                w_cluster_sets += (ull)__popcll(__ballot(tail));
            }
        }
    }
    if (bad) R.words[0] = 1;
    if (lane == 0) { sh_trace[wave][0] = w_kept; sh_trace[wave][1] = w_node_sets; sh_trace[wave][2] = w_cluster_sets; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ull kept = 0, node_sets = 0, cluster_sets = g_single;
        for (int w = 0; w < kWaves; ++w) { kept += sh_trace[w][0]; node_sets += sh_trace[w][1]; cluster_sets += sh_trace[w][2]; }
        if (kept) atomicAdd(&R.counts[0], kept);
        if (g_single) atomicAdd(&R.counts[1], g_single);
        if (cluster_sets) atomicAdd(&R.counts[2], cluster_sets);
        if (node_sets) atomicAdd(&R.counts[3], node_sets);
    }
}

// best[root] = the largest strength among the root's members.  A wave whose nodes carry one label (the usual case: node order is
// label order inside a big component) takes the maximum on chip and issues one atomic.
__global__ __launch_bounds__(kThreads) void k_report_best(const ReportArrays R, const u32 N) {
    const u32 lane = threadIdx.x & 63;
    const u64 n_pad = ((u64)N + 63) & ~63ull;   // whole waves take every step
    for (u64 v = (u64)blockIdx.x * kThreads + threadIdx.x; v < n_pad; v += (u64)gridDim.x * kThreads) {
        const bool node = v < N;
        const u32 L = node ? R.label[v] : kNone;
        u64 st = node ? (u64)R.strength[v] : 0;
        const u32 first = (u32)__shfl((int)L, 0);   // (lane 0 of a wave that holds a node holds one)
        if (__ballot(node && L != first) == 0) {
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {
                const u64 o = shfl_xor64(st, m);
                st = o > st ? o : st;
            }
            if (lane == 0 && st) atomicMax(&R.best[first], (ull)st);
        } else if (node && st) {
            atomicMax(&R.best[L], (ull)st);
        }
    }
}
// medoid[root] = the smallest member whose strength is the best (the slots start at 0xFFFFFFFF)
__global__ __launch_bounds__(kThreads) void k_report_medoid(const ReportArrays R, const u32 N) {
    for (u64 v = (u64)blockIdx.x * kThreads + threadIdx.x; v < N; v += (u64)gridDim.x * kThreads) {
        const u32 L = R.label[v];
        if ((ull)R.strength[v] == R.best[L]) atomicMin(&R.medoid[L], (u32)v);
    }
}
// via[v] = the lowest index of a kept record between v and the medoid of v's cluster (the slots start at 0xFFFFFFFF)
template <bool kRecords>
__global__ __launch_bounds__(kThreads) void k_report_links(const ReportIn in, const u64 n, const u64 n_chunks, const u32 N, const ReportArrays R) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = chunk * kChunk + (u64)wave * (kIters * 64);
        u32 s[kIters], t[kIters];
        float v[kIters];
        bool k[kIters];
#pragma unroll
        for (int i = 0; i < kIters; ++i) report_record<kRecords>(in, n, N, base + (u64)i * 64 + lane, s[i], t[i], v[i], k[i]);
#pragma unroll
        for (int i = 0; i < kIters; ++i) {
            if (!k[i]) continue;
            const u32 m = R.medoid[R.label[s[i]]];
            const u32 e = (u32)(base + (u64)i * 64 + lane);   // (an index is below 2^32 - 1: larger lists are refused)
            if (s[i] == m) atomicMin(&R.via[t[i]], e);        // (s != t: at most one end is the medoid)
            else if (t[i] == m) atomicMin(&R.via[s[i]], e);
        }
    }
}

// The times of the passes (ksp_debug_report_times), by HIP events on the null stream: a mark after every pass.
struct PassTimes {
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // around the accumulate pass (0, 1), the medoid passes (2, 3), the links pass (3, 4)
    float ms[3] = {0, 0, 0};
    ~PassTimes() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// The report on the CURRENT device over n > 0 edges and N > 0 nodes.  Nothing is written to the caller before everything has
// succeeded.
int report_on_device(const char* who, const u32 N, const ReportIn& in, const u64 n, ksp_cluster_row* h_cluster, u32* n_clusters, ksp_member_row* h_member,
                     ksp::ReportTrace& T, PassTimes* times) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::WorkgroupCap G;
    ReportArrays R;
    const u64 n_chunks = (n + kChunk - 1) / kChunk;
    const bool records = in.ed != nullptr;
    // One block, so that the call makes one allocation, two memsets and one copy back.  8-byte arrays first: strength, edges,
    // nan_edges, sum_q, best (N each), the counters (4) and the words (8 x 4 bytes); then deg, max (zeros up to here), via, min,
    // medoid (all ones) and the labels.  64 bytes per node and 64 more: the formula of the header.
    const size_t block_bytes = 64 * (size_t)N + 64, zero_bytes = 48 * (size_t)N + 64, ones_bytes = 12 * (size_t)N;
    unsigned char* d_block = nullptr;
    std::vector<u64> h_block;   // the block on the host (8-byte aligned)
    const u32 *label = nullptr, *deg = nullptr, *via = nullptr, *c_min = nullptr, *c_max = nullptr, *medoid = nullptr, *h_words = nullptr;
    const ull *strength = nullptr, *c_edges = nullptr, *c_nan = nullptr, *c_sumq = nullptr, *h_counts = nullptr;
    std::vector<u32> size, covered;
    std::vector<ksp_cluster_row> rows;
    auto mark = [&](const int i) { return times ? hipEventRecord(times->ev[i], nullptr) : hipSuccess; };
    // the arrays of a block that starts at `base`
    auto carve = [N](unsigned char* base, ReportArrays& X) {
        ull* p8 = reinterpret_cast<ull*>(base);
        X.strength = p8; X.c_edges = p8 + (size_t)N; X.c_nan = p8 + 2 * (size_t)N; X.c_sumq = p8 + 3 * (size_t)N; X.best = p8 + 4 * (size_t)N;
        X.counts = p8 + 5 * (size_t)N;
        u32* p4 = reinterpret_cast<u32*>(X.counts + 4);
        X.words = p4; p4 += 8;
        X.deg = p4; X.c_max = p4 + (size_t)N; X.via = p4 + 2 * (size_t)N; X.c_min = p4 + 3 * (size_t)N; X.medoid = p4 + 4 * (size_t)N; X.label = p4 + 5 * (size_t)N;
    };
    if ((rc = ksp::workgroup_cap("KSP_REPORT_MAX_WORKGROUPS", who, G))) return rc;
    const unsigned grid_nodes = G.grid_of(((u64)N + kThreads - 1) / kThreads), grid_edges = G.grid_of(n_chunks);
    // ---- everything the call holds, sized and checked first
    if ((rc = ksp::device_fits(who, block_bytes, "64 per node"))) return rc;
    if ((rc = A.alloc(&d_block, block_bytes))) return rc;
    carve(d_block, R);
    if (times)
        for (hipEvent_t& e : times->ev) KSP_TRY_HIP(hipEventCreate(&e));
    KSP_TRY_HIP(hipMemsetAsync(d_block, 0, zero_bytes, nullptr));
    KSP_TRY_HIP(hipMemsetAsync(d_block + zero_bytes, 0xFF, ones_bytes, nullptr));
    // ---- the labels: words[4 .. 7] are the rounds' scratch
    {
        ksp::CcRounds E;
        E.ed = in.ed; E.cnt = in.cnt; E.col = in.col; E.vcrit = in.vcrit; E.mode = in.mode; E.strict = true;
        E.a = in.a; E.b = in.b;
        if ((rc = ksp::cc_init_on_device(N, R.label)) || (rc = ksp::cc_rounds_on_device(E, N, n, R.label, R.words + 4, nullptr))) return rc;
    }
    KSP_TRY_HIP(mark(0));
    // ---- degree, strength and the clusters' sums
    if (records) hipLaunchKernelGGL(k_report_accumulate<true>, dim3(grid_edges), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, R);
    else hipLaunchKernelGGL(k_report_accumulate<false>, dim3(grid_edges), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, R);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(mark(1));
    // ---- the medoid of every cluster, then the records that link it to its members
    KSP_TRY_HIP(mark(2));
    hipLaunchKernelGGL(k_report_best, dim3(grid_nodes), dim3(kThreads), 0, nullptr, R, N);
    hipLaunchKernelGGL(k_report_medoid, dim3(grid_nodes), dim3(kThreads), 0, nullptr, R, N);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(mark(3));
    if (records) hipLaunchKernelGGL(k_report_links<true>, dim3(grid_edges), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, R);
    else hipLaunchKernelGGL(k_report_links<false>, dim3(grid_edges), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, R);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(mark(4));
    // ---- back to the host in one copy; the flag first (a refused call has run its last passes over sums without the bad values)
    h_block.resize(block_bytes / 8);
    KSP_TRY_HIP(hipMemcpy(h_block.data(), d_block, block_bytes, hipMemcpyDeviceToHost));
    {
        ReportArrays H;
        carve(reinterpret_cast<unsigned char*>(h_block.data()), H);
        label = H.label; deg = H.deg; via = H.via; c_min = H.c_min; c_max = H.c_max; medoid = H.medoid; h_words = H.words;
        strength = H.strength; c_edges = H.c_edges; c_nan = H.c_nan; c_sumq = H.c_sumq; h_counts = H.counts;
    }
    if (h_words[0]) {
        ksp::set_error(std::string(who) + ": a kept record's value lies outside [0, 1] (a containment above 1: shared k-mers above a source's count)");
        return KSP_E_ARG;
    }
    if (times)
        for (int i = 0; i < 3; ++i) KSP_TRY_HIP(hipEventElapsedTime(&times->ms[i], times->ev[i == 0 ? 0 : i + 1], times->ev[i == 0 ? 1 : i + 2]));
    // ---- sizes, covered, and the slots of the roots as rows in root order
    size.assign(N, 0); covered.assign(N, 0);
    for (u32 v = 0; v < N; ++v) {
        const u32 r = label[v];
        if (r > v || label[r] != r || medoid[r] >= N || label[medoid[r]] != r || (via[v] != kNone && via[v] >= n) || c_nan[r] > c_edges[r]) {
            ksp::set_error(std::string(who) + ": node " + std::to_string(v) + " was left without its cluster");
            return KSP_E_HIP;
        }
        ++size[r];
        covered[r] += via[v] != kNone;
    }
    for (u32 r = 0; r < N; ++r) {
        if (label[r] != r) continue;
        ksp_cluster_row c;
        const bool valued = c_edges[r] > c_nan[r];
        c.root = r; c.size = size[r];
        c.edges = c_edges[r]; c.nan_edges = c_nan[r]; c.sum_q = c_sumq[r];
        c.min = c.max = std::numeric_limits<float>::quiet_NaN();
        if (valued) { std::memcpy(&c.min, &c_min[r], 4); std::memcpy(&c.max, &c_max[r], 4); }
        c.medoid = medoid[r]; c.covered = covered[r];
        rows.push_back(c);
    }
    std::copy(rows.begin(), rows.end(), h_cluster);
    *n_clusters = (u32)rows.size();
    for (u32 v = 0; v < N; ++v) h_member[v] = ksp_member_row{label[v], deg[v], (u64)strength[v], via[v], 0u};
    T.kept = h_counts[0]; T.single_label_chunks = h_counts[1]; T.cluster_sets = h_counts[2]; T.node_sets = h_counts[3];
done:
    return rc;
}

// no record: every node is a singleton cluster and its own medoid
void report_empty(const u32 N, ksp_cluster_row* h_cluster, u32* n_clusters, ksp_member_row* h_member) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (u32 v = 0; v < N; ++v) {
        h_cluster[v] = ksp_cluster_row{v, 1u, 0, 0, 0, nan, nan, v, 0u};
        h_member[v] = ksp_member_row{v, 0u, 0, kNone, 0u};
    }
    *n_clusters = N;
}

int check_report_args(const char* who, const u32 n_nodes, const u64 n_edges, const bool null_input, const ksp_cluster_row* h_cluster, const u32* n_clusters,
                      const ksp_member_row* h_member) {
    if (!n_clusters || (n_nodes && (!h_cluster || !h_member)) || (n_edges && null_input)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 records or more (a record's index is `via`, and 0xFFFFFFFF is none)"); return KSP_E_LIMIT; }
    return KSP_OK;
}

int report_edges(const char* who, const u32 n_nodes, const ksp_edge* d_edges, const u64 n_edges, const u32* d_cnt, const int col, const double cutoff,
                 ksp_cluster_row* h_cluster, u32* n_clusters, ksp_member_row* h_member, ksp::ReportTrace* trace, PassTimes* times) {
    ksp::ReportTrace T;
    int rc = KSP_OK;
    if (n_edges == 0 || n_nodes == 0) {
        report_empty(n_nodes, h_cluster, n_clusters, h_member);   // no kernel runs
    } else {
        ReportIn in;
        in.ed = d_edges; in.cnt = d_cnt; in.col = col;
        ksp::cc_critical(cutoff, &in.vcrit, &in.mode);
        rc = report_on_device(who, n_nodes, in, n_edges, h_cluster, n_clusters, h_member, T, times);
    }
    g_trace = T;
    if (trace) *trace = T;
    return rc;
}

std::string g6(const double x) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.6g", x);
    return buf;
}
std::string float_text(const float x) {
    char buf[64];
    buf[ksp_format_float(x, buf)] = 0;
    return buf;
}

}  // namespace

namespace ksp {
int report_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, const double cutoff,
                           ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member, ReportTrace* trace) {
    if (const int rc = check_report_args("cluster report", n_nodes, n_edges, !d_edges || !d_cnt, h_cluster, n_clusters, h_member)) return rc;
    return report_edges("cluster report", n_nodes, d_edges, n_edges, d_cnt, col, cutoff, h_cluster, n_clusters, h_member, trace, nullptr);
}

void write_report_files(const std::string& prefix, const std::string& dist, const double threshold, const std::vector<ksp_cluster_row>& cluster,
                        const std::vector<ksp_member_row>& member, const std::vector<std::string>& via_text, const std::vector<std::string>& name_of) {
    const double two32 = 4294967296.0;
    const std::string tail = "_" + dist + "_" + py_float_repr(threshold) + "%.tsv";
    std::vector<u32> number_of(member.size(), 0);   // root -> the 1-based line of the cluster file
    for (size_t c = 0; c < cluster.size(); ++c) number_of[cluster[c].root] = (u32)c + 1;
    std::ofstream fc, fm;
    PartialFiles files;
    files.open(prefix + "_kSpider_cluster_report" + tail, fc);
    files.open(prefix + "_kSpider_cluster_members" + tail, fm);
    fc << "cluster\tsize\tedges\tdensity\tmin\tmean\tmax\tmedoid\tmedoid_strength\tcovered\n";
    for (size_t c = 0; c < cluster.size(); ++c) {
        const ksp_cluster_row& r = cluster[c];
        const u64 valued = r.edges - r.nan_edges;
        const double pairs = (double)r.size * ((double)r.size - 1.0) / 2.0;
        fc << c + 1 << '\t' << r.size << '\t' << r.edges << '\t' << (r.size > 1 ? g6((double)r.edges / pairs) : "-") << '\t' << (r.min != r.min ? "-" : float_text(r.min))
           << '\t' << (valued ? g6((double)r.sum_q / (double)valued / two32) : "-") << '\t' << (r.max != r.max ? "-" : float_text(r.max)) << '\t' << name_of[r.medoid]
           << '\t' << g6((double)member[r.medoid].strength / two32) << '\t' << r.covered << '\n';
    }
    fm << "source\tcluster\tmedoid\t" << dist << "\tneighbours\tstrength\n";
    for (size_t v = 0; v < member.size(); ++v) {
        const ksp_member_row& m = member[v];
        const ksp_cluster_row& r = cluster[number_of[m.label] - 1];
        fm << name_of[v] << '\t' << number_of[m.label] << '\t' << name_of[r.medoid] << '\t' << (m.via == kNone ? "-" : via_text[v]) << '\t' << m.degree << '\t'
           << g6((double)m.strength / two32) << '\n';
    }
    files.commit();
}
}  // namespace ksp

extern "C" int ksp_edges_cluster_report(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                        double cutoff, ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member) {
    const char* who = "ksp_edges_cluster_report";
    if (const int rc = check_report_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, h_cluster, n_clusters, h_member)) return rc;
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (cutoff != cutoff) { ksp::set_error(std::string(who) + ": the cut-off is NaN"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return report_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoff, h_cluster, n_clusters, h_member, nullptr, nullptr);
}

extern "C" int ksp_cluster_report_valued(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const float* h_value, uint64_t n_edges,
                                         ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member) {
    const char* who = "ksp_cluster_report_valued";
    if (const int rc = check_report_args(who, n_nodes, n_edges, !h_a || !h_b || !h_value, h_cluster, n_clusters, h_member)) return rc;
    for (u64 e = 0; e < n_edges; ++e)
        if (h_a[e] >= n_nodes || h_b[e] >= n_nodes) { ksp::set_error(std::string(who) + ": node index out of range"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    ksp::ReportTrace T;
    g_trace = T;
    if (n_edges == 0 || n_nodes == 0) { report_empty(n_nodes, h_cluster, n_clusters, h_member); return KSP_OK; }
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr;
    float* d_val = nullptr;
    ReportIn in;
    if ((rc = ksp::device_fits(who, 12ull * n_edges + 64ull * n_nodes + 64, "12 per valued edge, 64 per node"))) return rc;
    if ((rc = ksp::upload_pairs(A, h_a, h_b, n_edges, &d_a, &d_b)) || (rc = A.alloc(&d_val, (size_t)n_edges))) return rc;
    KSP_TRY_HIP(hipMemcpy(d_val, h_value, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    in.a = d_a; in.b = d_b; in.val = d_val;
    rc = report_on_device(who, n_nodes, in, n_edges, h_cluster, n_clusters, h_member, T, nullptr);
    g_trace = T;
done:
    return rc;
}

extern "C" int ksp_debug_report_counts(uint64_t out[4]) {
    if (!out) { ksp::set_error("ksp_debug_report_counts: NULL argument"); return KSP_E_ARG; }
    out[0] = g_trace.kept;
    out[1] = g_trace.single_label_chunks;
    out[2] = g_trace.cluster_sets;
    out[3] = g_trace.node_sets;
    return KSP_OK;
}

extern "C" int ksp_debug_report_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                      double cutoff, int reps, float* ms, ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member) {
    const char* who = "ksp_debug_report_times";
    if (!ms || reps < 1 || !n_nodes || !n_edges || dist_col < 3 || dist_col > 5 || cutoff != cutoff) { ksp::set_error(std::string(who) + ": bad argument"); return KSP_E_ARG; }
    if (const int rc = check_report_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, h_cluster, n_clusters, h_member)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<u32> labels(n_nodes);
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        PassTimes P;
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if ((rc = report_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoff, h_cluster, n_clusters, h_member, nullptr, &P))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[5 * r], ev0, ev1));
        for (int i = 0; i < 3; ++i) ms[5 * r + 1 + i] = P.ms[i];
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if ((rc = ksp::cc_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoff, labels.data(), nullptr))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[5 * r + 4], ev0, ev1));
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}

extern "C" int kspider_cluster_report(const char* index_prefix, const char* dist_type, double cutoff) {
    const char* who = "kspider_cluster_report";
    if (!index_prefix) { ksp::set_error(std::string(who) + ": index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (col < 3 || col > 5) {
        ksp::set_error(std::string(who) + ": distance '" + dt + "' is not min_cont, avg_cont or max_cont (a report sums containments in [0, 1])");
        return KSP_E_ARG;
    }
    if (!(cutoff >= 0 && cutoff <= 1)) { ksp::set_error(std::string(who) + ": the cut-off is not in [0, 1]"); return KSP_E_ARG; }
    const double threshold = cutoff * 100.0;   // (ks_clustering.py: cutoff = float(cutoff) * 100)
    g_trace = ksp::ReportTrace();
    try {
        std::vector<std::string> name_of, text;
        std::vector<u32> ea, eb;
        std::vector<float> value;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double d, const std::string& t) {
            if (d < threshold) return;   // (kspider_cluster's test on the text as it stands; a NaN is kept)
            ksp::check_row_nodes(a, b, name_of.size());
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            value.push_back(std::strtof(t.c_str(), nullptr));
            text.push_back(t);
        });
        const u64 N = name_of.size();
        std::vector<ksp_cluster_row> cluster((size_t)N + 1);
        std::vector<ksp_member_row> member((size_t)N + 1);
        u32 n_clusters = 0;
        const int rc = ksp_cluster_report_valued(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), value.data(), ea.size(), cluster.data(), &n_clusters, member.data());
        if (rc) return rc;
        cluster.resize(n_clusters);
        member.resize((size_t)N);
        std::vector<std::string> via_text((size_t)N);
        for (u64 v = 0; v < N; ++v)
            if (member[(size_t)v].via != kNone) via_text[(size_t)v] = text[member[(size_t)v].via];
        ksp::write_report_files(prefix, dt, threshold, cluster, member, via_text, name_of);
        if (std::getenv("KSPIDER_VERBOSE")) {
            const ksp_cluster_row* big = nullptr;
            for (const ksp_cluster_row& c : cluster)
                if (!big || c.size > big->size) big = &c;
            std::cout << "kspider_amd: cluster report: " << ea.size() << " records kept, " << cluster.size() << " clusters";
            if (big) std::cout << ", the largest of " << big->size << " sources, density " << (big->size > 1 ? g6((double)big->edges / ((double)big->size * (big->size - 1.0) / 2.0)) : "-");
            std::cout << std::endl;
        }
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}
