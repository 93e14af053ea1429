// Top-k neighbours: for every source its k best hits among the join's edge records while they are in HBM, or
// among the ranked rows of an existing TSV — the one consumer whose result is bounded (n_nodes x k) however dense the graph is.
//
// Definition.
//   entries   an entry of node v is a record that names v and is no self pair (source_1 != source_2).  Every such record is
//             an entry of BOTH of its ends, whatever its `shared`; a pair that repeats is listed again; a record naming a node
//             >= n_nodes is the caller's error and is ignored, as in ksp_components_edges.
//   order     the entries of v by (1) value descending, (2) a NaN below every number — a source without k-mers is never
//             somebody's best hit; the tree (tree.hip) puts a NaN on top because a NaN row is kept at every cut-off, here the
//             opposite is right — (3) ties by record index, lower first.  A strict total order: the result is unique and does
//             not depend on how the device arranges a node's entries.
//   value     the float of column 3, 4 or 5 in single precision exactly as the pairwise writer and the sibling consumers
//             compute it (edge_cut.hip.h = src/pairwise.cpp:260-264); +inf is a number and sorts first.  No value is negative.
//   result    count[v] = min(k, entries of v); index[v * k + i], i < count[v], = the record index of the i-th entry in that
//             order; every slot behind count[v] is 0xFFFFFFFF.
//
//   count     k_topk_count: entries per node.  Consecutive lanes of a wave that name the same node (the join's records are
//             sorted by source_1) share one atomic.
//   scan      rocPRIM's exclusive scan over the nodes, 64-bit offsets: there are up to 2 x n_edges entries
//   scatter   k_topk_scatter: every record writes one 64-bit key into the segment of each of its ends, at a position taken
//             from a per-node cursor (32-bit atomic).  High half: the value as an unsigned integer that sorts in the order
//             above (topk_value_key; the ranked form: ~rank), low half: the record index.  Ascending keys = best first; the
//             arrangement inside a segment is arbitrary.  An all-ones key is no entry (an index is below 2^32 - 1).
//   classify  k_topk_classify: count[v], and every node with entries appended to one of three lists, one append per wave and
//             list; the class depends on the number of entries n and on nothing else
//   select    n <= KSP_TOPK_WAVE_ENTRIES   k_topk_select_wave: one wave per node, one key per lane, a bitonic network of
//                                          cross-lane exchanges (no LDS round trip, no barrier)
//             n <= KSP_TOPK_LDS_ENTRIES    k_topk_select_wg: one workgroup per node, the segment in LDS padded with all-ones
//                                          keys to a power of two, a bitonic sort there
//             larger                       k_topk_select_stream: one workgroup per node; the best k so far stay sorted at the
//                                          head of the LDS buffer, the other KSP_TOPK_LDS_ENTRIES - k slots are refilled from
//                                          the segment (all loads of a refill in flight before the first is used; a key that is
//                                          not better than the current k-th is dropped at load), sorted in; a refill that lets
//                                          no key through is not sorted
//   $KSP_TOPK_SELECT=library (tests and timing): rocprim::segmented_radix_sort_keys over all segments, k_topk_gather takes
//             the first k of each.  The same result by definition.
// Every edge pass owns chunks of KSP_TOPK_CHUNK_EDGES consecutive records per workgroup, as cut.hip and derep.hip do; no
// workgroup ever waits on another, and every loop is bounded by a size the host computed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/kspider_amd.h"
#include "cluster_inputs.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kTopkChunk = KSP_TOPK_CHUNK_EDGES;   // (the reasons for 2 048 entries per 256 threads: cut.hip)
constexpr int kTopkThreads = 256;
constexpr int kTopkWaves = kTopkThreads / 64;
constexpr int kTopkIters = (int)(kTopkChunk / kTopkThreads);   // records per lane and chunk
constexpr u32 kLds = KSP_TOPK_LDS_ENTRIES;
constexpr int kRefillPerThread = (int)(kLds / kTopkThreads);   // keys a thread loads per refill, at most
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr u64 kPad = ~0ull;   // no entry: above every key
static_assert(kTopkIters * kTopkThreads == (int)kTopkChunk, "a chunk is whole ballots of every wave");
static_assert(KSP_TOPK_WAVE_ENTRIES == 64, "the wave kernel holds one key per lane");
static_assert((kLds & (kLds - 1)) == 0 && kLds % kTopkThreads == 0, "the LDS buffer is sorted as a whole");
static_assert(2 * KSP_TOPK_MAX_K <= KSP_TOPK_LDS_ENTRIES, "a refill brings at least as many keys as stay");
static_assert(2 * kLds * sizeof(u64) <= 160 * 1024, "two workgroups per CU");

thread_local ksp::TopkTrace g_trace;   // (ksp_debug_topk_classes)

enum SelectMode { kFromEnv = -1, kKernels = 0, kLibrary = 1 };

// the edges of one call: the join's records (ed, cnt, col) or ranked pairs (a, b, rank)
struct TopkIn {
    const ksp_edge* ed = nullptr;
    const u32* cnt = nullptr;
    int col = 0;
    const u32 *a = nullptr, *b = nullptr, *rank = nullptr;
};

// first record of wave `wave` in chunk `chunk`: wave w owns the records [w * 512, (w + 1) * 512) of its chunk
__device__ inline u64 topk_wave_base(const u64 chunk, const u32 wave) { return chunk * kTopkChunk + (u64)wave * (kTopkIters * 64); }

// The high half of a key: larger values get smaller words, a NaN the largest.  (A float's bits with the sign flipped, or all
// bits flipped below zero, ascend with the value; the complement descends.)
__device__ inline u32 topk_value_key(const float v) {
    if (v != v) return 0xFFFFFFFFu;
    u32 b = __float_as_uint(v);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ~b;
}

// The ends of a chunk's records into registers, all loads in flight before the first is used.  kRecords: the join's records
// (w = `shared`); else ranked pairs (w = the rank).
template <bool kRecords>
__device__ inline void topk_load(const TopkIn& in, const u64 n, const u64 base, const u32 lane, u32 (&s)[kTopkIters], u32 (&t)[kTopkIters],
                                 u64 (&w)[kTopkIters]) {
#pragma unroll
    for (int i = 0; i < kTopkIters; ++i) {
        const u64 e = base + (u64)i * 64 + lane;
        s[i] = t[i] = kNone;
        w[i] = 0;
        if (e < n) {
            if (kRecords) {
                const ksp_edge x = in.ed[e];
                s[i] = x.source_1; t[i] = x.source_2; w[i] = x.shared;
            } else {
                s[i] = in.a[e]; t[i] = in.b[e]; w[i] = in.rank[e];
            }
        }
    }
}
// a record is an entry of both ends when both are nodes and it is no self pair (an end of kNone is never below n_nodes)
__device__ inline bool topk_is_entry(const u32 s, const u32 t, const u32 n_nodes) { return s < n_nodes && t < n_nodes && s != t; }

// counter[v] += 1 for every lane with v != kNone; returns what the lane's own atomic would have returned.  Consecutive lanes
// that hold the same v make ONE atomic of their run's length.  Every lane of the wave calls it.
__device__ inline u32 topk_run_add(u32* counter, const u32 v, const u32 lane) {
    const u32 prev = (u32)__shfl_up((int)v, 1);
    const bool head = lane == 0 || prev != v;
    const unsigned long long heads = __ballot(head);
    const u32 start = 63u - (u32)__clzll((long long)(heads & (~0ull >> (63 - lane))));   // the first lane of my run
    const unsigned long long after = lane == 63 ? 0ull : heads >> (lane + 1);
    const u32 end = after ? lane + (u32)__ffsll(after) : 64u;                             // the first lane behind it
    u32 base = 0;
    if (head && v != kNone) base = atomicAdd(&counter[v], end - start);
    base = (u32)__shfl((int)base, (int)start);
    return base + (lane - start);
}

template <bool kRecords>
__global__ __launch_bounds__(kTopkThreads) void k_topk_count(const TopkIn in, const u64 n, const u64 n_chunks, const u32 n_nodes, u32* __restrict__ deg) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        u32 s[kTopkIters], t[kTopkIters];
        u64 w[kTopkIters];
        topk_load<kRecords>(in, n, topk_wave_base(chunk, wave), lane, s, t, w);
#pragma unroll
        for (int i = 0; i < kTopkIters; ++i) {
            const bool entry = topk_is_entry(s[i], t[i], n_nodes);
            topk_run_add(deg, entry ? s[i] : kNone, lane);
            topk_run_add(deg, entry ? t[i] : kNone, lane);
        }
    }
}

// The same chunks again: key (value word, record index) into the segment of both ends.  A position that is not inside the
// segment the count pass sized (the records changed under the call) is not written.
template <bool kRecords>
__global__ __launch_bounds__(kTopkThreads) void k_topk_scatter(const TopkIn in, const u64 n, const u64 n_chunks, const u32 n_nodes,
                                                               const u64* __restrict__ off, u32* __restrict__ cursor, u64* __restrict__ keys) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = topk_wave_base(chunk, wave);
        u32 s[kTopkIters], t[kTopkIters];
        u64 w[kTopkIters];
        topk_load<kRecords>(in, n, base, lane, s, t, w);
#pragma unroll
        for (int i = 0; i < kTopkIters; ++i) {
            const bool entry = topk_is_entry(s[i], t[i], n_nodes);
            const u32 ps = topk_run_add(cursor, entry ? s[i] : kNone, lane);
            const u32 pt = topk_run_add(cursor, entry ? t[i] : kNone, lane);
            if (!entry) continue;
            const u32 hi = kRecords ? topk_value_key(edge_col_value(ksp_edge{s[i], t[i], w[i]}, in.cnt, in.col)) : ~(u32)w[i];
            const u64 key = ((u64)hi << 32) | (u32)(base + (u64)i * 64 + lane);   // (an index is below 2^32 - 1: larger lists are refused)
            const u64 os = off[s[i]], ot = off[t[i]];
            if (os + ps < off[s[i] + 1]) keys[os + ps] = key;
            if (ot + pt < off[t[i] + 1]) keys[ot + pt] = key;
        }
    }
}

// count[v] = min(k, entries), and v into the list of its class: one append per wave and list
__global__ void k_topk_classify(const u32* __restrict__ deg, const u32 n_nodes, const u32 k, u32* __restrict__ count, u32* __restrict__ list_wave,
                                u32* __restrict__ list_wg, u32* __restrict__ list_stream, u32* __restrict__ n_list) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    const u32 n = v < n_nodes ? deg[v] : 0;
    if (v < n_nodes) count[v] = n < k ? n : k;
    const int cls = n == 0 ? -1 : n <= KSP_TOPK_WAVE_ENTRIES ? 0 : n <= kLds ? 1 : 2;
    u32* const lists[3] = {list_wave, list_wg, list_stream};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned long long b = __ballot(cls == c);
        u32 base = 0;
        if (lane == 0 && b) base = atomicAdd(&n_list[c], (u32)__popcll(b));
        base = (u32)__shfl((int)base, 0);
        if (cls == c) lists[c][base + (u32)__popcll(b & ((1ull << lane) - 1))] = (u32)v;
    }
}

__device__ inline u64 topk_shfl_xor(const u64 x, const int mask) {
    const u32 lo = (u32)__shfl_xor((int)(u32)x, mask), hi = (u32)__shfl_xor((int)(u32)(x >> 32), mask);
    return ((u64)hi << 32) | lo;
}

// One wave per node of at most 64 entries: a bitonic network over the lanes, then the first min(k, n) lanes write.
__global__ __launch_bounds__(kTopkThreads) void k_topk_select_wave(const u32* __restrict__ list, const u32 n_list, const u64* __restrict__ off,
                                                                   const u64* __restrict__ keys, const u32 k, u32* __restrict__ index) {
    const u32 lane = threadIdx.x & 63;
    for (u64 i = (u64)blockIdx.x * kTopkWaves + (threadIdx.x >> 6); i < n_list; i += (u64)gridDim.x * kTopkWaves) {
        const u32 v = list[i];
        const u64 o = off[v];
        const u32 n = (u32)std::min<u64>(off[v + 1] - o, 64);   // (the class's bound)
        u64 key = lane < n ? keys[o + lane] : kPad;
#pragma unroll
        for (u32 size = 2; size <= 64; size <<= 1) {
#pragma unroll
            for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
                const u64 other = topk_shfl_xor(key, (int)stride);
                const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);   // (size 64: every lane ascends)
                key = keep_min ? (other < key ? other : key) : (other > key ? other : key);
            }
        }
        if (lane < (n < k ? n : k)) index[(u64)v * k + lane] = (u32)key;
    }
}

// Ascending bitonic sort of buf[0 .. P) in LDS by the whole workgroup, P a power of two; a barrier before every pass and one
// behind the last.
__device__ inline void topk_lds_sort(u64* buf, const u32 P) {
    for (u32 size = 2; size <= P; size <<= 1) {
        for (u32 stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (u32 t = threadIdx.x; t < P / 2; t += kTopkThreads) {
                const u32 i = 2 * t - (t & (stride - 1)), j = i + stride;   // pair t of the pass: t with a 0 bit inserted at `stride`
                const u64 x = buf[i], y = buf[j];
                if ((x > y) == ((i & size) == 0)) { buf[i] = y; buf[j] = x; }
            }
        }
    }
    __syncthreads();
}

// One workgroup per node of at most KSP_TOPK_LDS_ENTRIES entries: the segment in LDS, padded to a power of two, sorted there.
__global__ __launch_bounds__(kTopkThreads) void k_topk_select_wg(const u32* __restrict__ list, const u32 n_list, const u64* __restrict__ off,
                                                                 const u64* __restrict__ keys, const u32 k, u32* __restrict__ index) {
    __shared__ u64 buf[kLds];
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const u32 v = list[i];
        const u64 o = off[v];
        const u32 n = (u32)std::min<u64>(off[v + 1] - o, kLds);   // (the class's bound)
        const u32 P = n <= 2 ? 2u : 1u << (32 - __clz((int)(n - 1)));
        for (u32 j = threadIdx.x; j < P; j += kTopkThreads) buf[j] = j < n ? keys[o + j] : kPad;
        topk_lds_sort(buf, P);
        const u32 m = n < k ? n : k;
        for (u32 j = threadIdx.x; j < m; j += kTopkThreads) index[(u64)v * k + j] = (u32)buf[j];
        __syncthreads();   // (buf is filled again for the next node)
    }
}

// One workgroup per node of any number of entries.  buf[0 .. k): the best k so far, sorted (all-ones while there are fewer);
// buf[k .. kLds): the slots of a refill.  *refills += the refills of every node.
__global__ __launch_bounds__(kTopkThreads) void k_topk_select_stream(const u32* __restrict__ list, const u32 n_list, const u64* __restrict__ off,
                                                                     const u64* __restrict__ keys, const u32 k, u32* __restrict__ index,
                                                                     unsigned long long* __restrict__ refills) {
    __shared__ u64 buf[kLds];
    const u32 room = kLds - k;   // (at least half of the buffer: k <= KSP_TOPK_MAX_K)
    for (u64 i = blockIdx.x; i < n_list; i += gridDim.x) {
        const u32 v = list[i];
        const u64 o = off[v], n = off[v + 1] - o;
        for (u32 j = threadIdx.x; j < k; j += kTopkThreads) buf[j] = kPad;
        __syncthreads();
        u32 fills = 0;
        for (u64 done = 0; done < n; done += room) {
            const u64 worst = buf[k - 1];   // the current k-th: nothing writes it before the sort's first barrier
            u64 r[kRefillPerThread];
#pragma unroll
            for (int q = 0; q < kRefillPerThread; ++q) {
                const u32 j = (u32)q * kTopkThreads + threadIdx.x;
                r[q] = (j < room && done + j < n) ? keys[o + done + j] : kPad;
            }
            int passed = 0;
#pragma unroll
            for (int q = 0; q < kRefillPerThread; ++q) {
                const u32 j = (u32)q * kTopkThreads + threadIdx.x;
                const bool better = r[q] < worst;
                passed |= (int)better;
                if (j < room) buf[k + j] = better ? r[q] : kPad;
            }
            if (__syncthreads_or(passed)) topk_lds_sort(buf, kLds);   // (no key passed: the head is what it was)
            ++fills;
        }
        const u32 m = (u32)std::min<u64>(n, k);
        for (u32 j = threadIdx.x; j < m; j += kTopkThreads) index[(u64)v * k + j] = (u32)buf[j];
        if (threadIdx.x == 0) atomicAdd(refills, (unsigned long long)fills);
        __syncthreads();   // (buf is filled again for the next node)
    }
}

// (library mode) count[v] and the first min(k, entries) keys of every sorted segment
__global__ void k_topk_gather(const u64* __restrict__ off, const u64* __restrict__ sorted, const u32 n_nodes, const u32 k, u32* __restrict__ index,
                              u32* __restrict__ count) {
    const u64 slots = (u64)n_nodes * k;
    for (u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; x < slots; x += (u64)gridDim.x * blockDim.x) {
        const u32 v = (u32)(x / k), j = (u32)(x % k);
        const u64 o = off[v], n = off[v + 1] - o;
        if (j == 0) count[v] = (u32)std::min<u64>(n, k);
        if (j < n) index[x] = (u32)sorted[o + j];
    }
}

struct ToU64 {
    __host__ __device__ u64 operator()(const u32 x) const { return x; }
};

int select_mode_from_env(const char* who, int* mode) {
    const char* s = std::getenv("KSP_TOPK_SELECT");
    if (!s || !*s || std::strcmp(s, "kernels") == 0) *mode = kKernels;
    else if (std::strcmp(s, "library") == 0) *mode = kLibrary;
    else { ksp::set_error(std::string(who) + ": KSP_TOPK_SELECT is 'kernels' or 'library'"); return KSP_E_ARG; }
    return KSP_OK;
}

template <class Kernel, class... Args>
void launch_edge_pass(Kernel kernel, const ksp::WorkgroupCap& G, const u64 n_chunks, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(G.grid_of(n_chunks)), dim3(kTopkThreads), 0, nullptr, args...);
}

// The selection on the CURRENT device over n > 0 edges and N > 0 nodes, 1 <= k <= KSP_TOPK_MAX_K.  Nothing is written to the
// caller before everything has succeeded.
int topk_on_device(const char* who, const u32 N, const TopkIn& in, const u64 n, const u32 k, int mode, u32* h_index, u32* h_count, ksp::TopkTrace& T) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::WorkgroupCap G;   // of the edge passes and of the select kernels, whose workgroups loop over their lists
    const u64 n_chunks = (n + kTopkChunk - 1) / kTopkChunk;
    const unsigned gn = (unsigned)(((u64)N + 255) / 256);
    const bool records = in.ed != nullptr;
    u32 *deg = nullptr, *cursor = nullptr, *lists[3] = {nullptr, nullptr, nullptr}, *count = nullptr, *index = nullptr, *n_list = nullptr;
    u64 *off = nullptr, *keys = nullptr, *sorted = nullptr;
    unsigned long long* refills = nullptr;
    void* tmp = nullptr;
    size_t tb_scan = 0;
    u64 total = 0;
    u32 h_lists[3] = {0, 0, 0};
    unsigned long long h_refills = 0;
    std::vector<u32> st_index, st_count;
    if (mode == kFromEnv && (rc = select_mode_from_env(who, &mode))) return rc;
    if ((rc = ksp::workgroup_cap("KSP_TOPK_MAX_WORKGROUPS", who, G))) return rc;
    const auto in_u64 = rocprim::make_transform_iterator((const u32*)nullptr, ToU64());
    // ---- everything the call holds, sized and checked first: 16 bytes per record (a key per entry, two entries per record),
    // 32 + 4 k per node (entries 4, offset 8, cursor 4, three lists 12, count 4, k indices), the scan's scratch
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, in_u64, (u64*)nullptr, (u64)0, (size_t)N + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
    tb_scan = std::max<size_t>(tb_scan, 8);
    if ((rc = ksp::device_fits(who, 16ull * n + (32ull + 4ull * k) * N + 64 + tb_scan, "16 per record, 32 + 4 k per node, the scan's scratch"))) return rc;
    if ((rc = A.alloc(&deg, (size_t)N + 1)) || (rc = A.alloc(&off, (size_t)N + 1)) || (rc = A.alloc(&cursor, (size_t)N)) || (rc = A.alloc(&count, (size_t)N))) return rc;
    for (u32*& l : lists)
        if ((rc = A.alloc(&l, (size_t)N))) return rc;
    if ((rc = A.alloc(&index, (size_t)N * k)) || (rc = A.alloc(&n_list, 4)) || (rc = A.alloc(&refills, 1)) || (rc = A.alloc_bytes(&tmp, tb_scan))) return rc;
    KSP_TRY_HIP(hipMemsetAsync(deg, 0, ((size_t)N + 1) * 4, nullptr));
    KSP_TRY_HIP(hipMemsetAsync(cursor, 0, (size_t)N * 4, nullptr));
    KSP_TRY_HIP(hipMemsetAsync(n_list, 0, 16, nullptr));
    KSP_TRY_HIP(hipMemsetAsync(refills, 0, 8, nullptr));
    KSP_TRY_HIP(hipMemsetAsync(index, 0xFF, (size_t)N * k * 4, nullptr));
    // ---- entries per node and their offsets
    if (records) launch_edge_pass(k_topk_count<true>, G, n_chunks, in, n, n_chunks, N, deg);
    else launch_edge_pass(k_topk_count<false>, G, n_chunks, in, n, n_chunks, N, deg);
    KSP_TRY_HIP(hipGetLastError());
    {
        size_t tb = tb_scan;
        KSP_TRY_HIP(rocprim::exclusive_scan(tmp, tb, rocprim::make_transform_iterator((const u32*)deg, ToU64()), off, (u64)0, (size_t)N + 1, rocprim::plus<u64>(),
                                            (hipStream_t) nullptr));
    }
    KSP_TRY_HIP(hipMemcpy(&total, off + N, 8, hipMemcpyDeviceToHost));
    if (total > 2 * n) { ksp::set_error(std::string(who) + ": more entries than two per record"); return KSP_E_HIP; }
    if (total) {
        // ---- the keys of every segment
        if ((rc = A.alloc(&keys, (size_t)total))) return rc;
        if (records) launch_edge_pass(k_topk_scatter<true>, G, n_chunks, in, n, n_chunks, N, (const u64*)off, cursor, keys);
        else launch_edge_pass(k_topk_scatter<false>, G, n_chunks, in, n, n_chunks, N, (const u64*)off, cursor, keys);
        KSP_TRY_HIP(hipGetLastError());
    }
    if (mode == kLibrary) {
        if (total >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": KSP_TOPK_SELECT=library sorts fewer than 2^32 - 1 entries"); return KSP_E_LIMIT; }
        if (total) {
            size_t tb_sort = 0;
            void* tmp_sort = nullptr;
            KSP_TRY_HIP(rocprim::segmented_radix_sort_keys(nullptr, tb_sort, (const u64*)keys, (u64*)nullptr, (unsigned)total, N, (const u64*)off, (const u64*)off + 1, 0, 64,
                                                           (hipStream_t) nullptr));
            tb_sort = std::max<size_t>(tb_sort, 8);
            if ((rc = ksp::device_fits(who, 8ull * total + tb_sort, "library mode: a second key per entry and the sort's scratch"))) return rc;
            if ((rc = A.alloc(&sorted, (size_t)total)) || (rc = A.alloc_bytes(&tmp_sort, tb_sort))) return rc;
            KSP_TRY_HIP(rocprim::segmented_radix_sort_keys(tmp_sort, tb_sort, (const u64*)keys, sorted, (unsigned)total, N, (const u64*)off, (const u64*)off + 1, 0, 64,
                                                           (hipStream_t) nullptr));
        }
        hipLaunchKernelGGL(k_topk_gather, dim3(G.grid_of(((u64)N * k + 255) / 256)), dim3(256), 0, nullptr, (const u64*)off, (const u64*)sorted, N, k, index, count);
        KSP_TRY_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_topk_classify, dim3(gn), dim3(256), 0, nullptr, (const u32*)deg, N, k, count, lists[0], lists[1], lists[2], n_list);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipMemcpy(h_lists, n_list, 12, hipMemcpyDeviceToHost));
        if ((u64)h_lists[0] + h_lists[1] + h_lists[2] > N) { ksp::set_error(std::string(who) + ": more classified nodes than nodes"); return KSP_E_HIP; }
        if (h_lists[0])
            hipLaunchKernelGGL(k_topk_select_wave, dim3(G.grid_of(((u64)h_lists[0] + kTopkWaves - 1) / kTopkWaves)), dim3(kTopkThreads), 0, nullptr, (const u32*)lists[0],
                               h_lists[0], (const u64*)off, (const u64*)keys, k, index);
        if (h_lists[1])
            hipLaunchKernelGGL(k_topk_select_wg, dim3(G.grid_of(h_lists[1])), dim3(kTopkThreads), 0, nullptr, (const u32*)lists[1], h_lists[1], (const u64*)off,
                               (const u64*)keys, k, index);
        if (h_lists[2])
            hipLaunchKernelGGL(k_topk_select_stream, dim3(G.grid_of(h_lists[2])), dim3(kTopkThreads), 0, nullptr, (const u32*)lists[2], h_lists[2], (const u64*)off,
                               (const u64*)keys, k, index, refills);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipMemcpy(&h_refills, refills, 8, hipMemcpyDeviceToHost));
    }
    st_index.resize((size_t)N * k);
    st_count.resize(N);
    KSP_TRY_HIP(hipMemcpy(st_index.data(), index, (size_t)N * k * 4, hipMemcpyDeviceToHost));
    KSP_TRY_HIP(hipMemcpy(st_count.data(), count, (size_t)N * 4, hipMemcpyDeviceToHost));
    for (u32 v = 0; v < N; ++v)
        if (st_count[v] > k || (st_count[v] && st_index[(size_t)v * k + st_count[v] - 1] >= n)) {
            ksp::set_error(std::string(who) + ": node " + std::to_string(v) + " was left without its hits");
            return KSP_E_HIP;
        }
    std::memcpy(h_index, st_index.data(), (size_t)N * k * 4);
    std::memcpy(h_count, st_count.data(), (size_t)N * 4);
    T.wave = h_lists[0]; T.workgroup = h_lists[1]; T.stream = h_lists[2]; T.refills = h_refills;
done:
    return rc;
}

// no record: no node has an entry
void topk_empty(const u32 N, const u32 k, u32* h_index, u32* h_count) {
    if (N) std::memset(h_index, 0xFF, (size_t)N * k * 4);
    for (u32 v = 0; v < N; ++v) h_count[v] = 0;
}

int check_topk_args(const char* who, const u32 n_nodes, const u64 n_edges, const bool null_input, const u32 k, const u32* h_index, const u32* h_count) {
    if (!h_count || (n_nodes && !h_index) || (n_edges && null_input)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (k == 0 || k > KSP_TOPK_MAX_K) { ksp::set_error(std::string(who) + ": k is 1 .. " + std::to_string(KSP_TOPK_MAX_K)); return KSP_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 records or more (a record's index is half of its 64-bit key)"); return KSP_E_LIMIT; }
    return KSP_OK;
}

int topk_edges(const char* who, const u32 n_nodes, const ksp_edge* d_edges, const u64 n_edges, const u32* d_cnt, const int col, const u32 k, const int mode,
               u32* h_index, u32* h_count, ksp::TopkTrace* trace) {
    ksp::TopkTrace T;
    int rc = KSP_OK;
    if (n_edges == 0 || n_nodes == 0) {
        topk_empty(n_nodes, k, h_index, h_count);   // no kernel runs
    } else {
        TopkIn in;
        in.ed = d_edges; in.cnt = d_cnt; in.col = col;
        rc = topk_on_device(who, n_nodes, in, n_edges, k, mode, h_index, h_count, T);
    }
    g_trace = T;
    if (trace) *trace = T;
    return rc;
}

}  // namespace

namespace ksp {
int topk_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, const uint32_t k,
                         uint32_t* h_index, uint32_t* h_count, TopkTrace* trace) {
    return topk_edges("topk", n_nodes, d_edges, n_edges, d_cnt, col, k, kFromEnv, h_index, h_count, trace);
}

// "source\thit\tneighbour\t<dist>" and one row per hit — the sources in the order of the names, their hits 1, 2, ... — through
// out_path.partial and a rename; on a failure nothing is left behind.  count: hits per name; neighbour / text: all hits, flat.
void write_topk_file(const std::string& out_path, const std::string& dist, const std::vector<std::string>& name_of, const std::vector<uint32_t>& count,
                     const std::vector<uint32_t>& neighbour, const std::vector<std::string>& text) {
    std::ofstream f;
    PartialFiles files;
    files.open(out_path, f);
    f << "source\thit\tneighbour\t" << dist << "\n";
    size_t h = 0;
    for (size_t v = 0; v < name_of.size(); ++v)
        for (uint32_t i = 0; i < count[v]; ++i, ++h) f << name_of[v] << '\t' << i + 1 << '\t' << name_of[neighbour[h]] << '\t' << text[h] << '\n';
    files.commit();
}
}  // namespace ksp

extern "C" int ksp_edges_topk(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, uint32_t k,
                              uint32_t* h_index, uint32_t* h_count) {
    const char* who = "ksp_edges_topk";
    if (const int rc = check_topk_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, k, h_index, h_count)) return rc;
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return topk_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, k, kFromEnv, h_index, h_count, nullptr);
}

extern "C" int ksp_topk_ranked(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_rank, uint64_t n_edges, uint32_t k,
                               uint32_t* h_index, uint32_t* h_count) {
    const char* who = "ksp_topk_ranked";
    if (const int rc = check_topk_args(who, n_nodes, n_edges, !h_a || !h_b || !h_rank, k, h_index, h_count)) return rc;
    for (u64 e = 0; e < n_edges; ++e)
        if (h_a[e] >= n_nodes || h_b[e] >= n_nodes) { ksp::set_error(std::string(who) + ": node index out of range"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    ksp::TopkTrace T;
    g_trace = T;
    if (n_edges == 0 || n_nodes == 0) { topk_empty(n_nodes, k, h_index, h_count); return KSP_OK; }
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr, *d_rank = nullptr;
    TopkIn in;
    if ((rc = ksp::device_fits(who, 12ull * n_edges, "12 per ranked edge"))) return rc;
    if ((rc = ksp::upload_pairs(A, h_a, h_b, n_edges, &d_a, &d_b)) || (rc = A.alloc(&d_rank, (size_t)n_edges))) return rc;
    KSP_TRY_HIP(hipMemcpy(d_rank, h_rank, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    in.a = d_a; in.b = d_b; in.rank = d_rank;
    rc = topk_on_device(who, n_nodes, in, n_edges, k, kFromEnv, h_index, h_count, T);
    g_trace = T;
done:
    return rc;
}

extern "C" int ksp_debug_topk_classes(uint64_t out[4]) {
    if (!out) { ksp::set_error("ksp_debug_topk_classes: NULL argument"); return KSP_E_ARG; }
    out[0] = g_trace.wave;
    out[1] = g_trace.workgroup;
    out[2] = g_trace.stream;
    out[3] = g_trace.refills;
    return KSP_OK;
}

// (tools/topk_times.py) HIP-event times of `reps` runs of ksp_edges_topk's device part over the same records: which 0 = the
// hand-written select kernels, 1 = rocPRIM's segmented sort.  Each time covers everything the call does on the device, its
// allocations and the copy of the result to the host included.  ms[reps].
extern "C" int ksp_debug_topk_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                    uint32_t k, int which, int reps, float* ms, uint32_t* h_index, uint32_t* h_count) {
    const char* who = "ksp_debug_topk_times";
    if (!ms || reps < 1 || which < 0 || which > 1 || !n_nodes || dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": bad argument"); return KSP_E_ARG; }
    if (const int rc = check_topk_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, k, h_index, h_count)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if ((rc = topk_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, k, which, h_index, h_count, nullptr))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}

extern "C" int kspider_topk(const char* index_prefix, const char* dist_type, uint32_t k, const char* out_path) {
    const char* who = "kspider_topk";
    if (!index_prefix) { ksp::set_error(std::string(who) + ": index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (!col) { ksp::set_error(std::string(who) + ": unknown distance '" + dt + "' (min_cont, avg_cont, max_cont, ani)"); return KSP_E_ARG; }
    if (k == 0 || k > KSP_TOPK_MAX_K) { ksp::set_error(std::string(who) + ": k is 1 .. " + std::to_string(KSP_TOPK_MAX_K)); return KSP_E_ARG; }
    g_trace = ksp::TopkTrace();
    try {
        std::vector<std::string> name_of, text;
        std::vector<u32> ea, eb;
        std::vector<double> weight;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double, const std::string& t) {
            ksp::check_row_nodes(a, b, name_of.size());   // every row is an entry of its two sources
            double w = 0;
            parse_float(t, w);   // (the reader has checked that the text is a number)
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            weight.push_back(w);
            text.push_back(t);
        });
        const u64 N = name_of.size(), n = ea.size();
        // doubles do not fit the device's key: the distinct weights, sorted, become the ranks 1, 2, ...; a NaN is rank 0, the lowest
        std::vector<double> distinct;
        for (const double w : weight)
            if (w == w) distinct.push_back(w);
        std::sort(distinct.begin(), distinct.end());
        distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
        std::vector<u32> rank((size_t)n);
        for (u64 e = 0; e < n; ++e)
            rank[(size_t)e] = weight[(size_t)e] != weight[(size_t)e] ? 0u : 1u + (u32)(std::lower_bound(distinct.begin(), distinct.end(), weight[(size_t)e]) - distinct.begin());
        std::vector<u32> index((size_t)N * k + 1), count((size_t)N + 1);
        const int rc = ksp_topk_ranked(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), rank.data(), n, k, index.data(), count.data());
        if (rc) return rc;
        count.resize((size_t)N);
        std::vector<u32> neighbour;
        std::vector<std::string> hit_text;
        for (u64 v = 0; v < N; ++v)
            for (u32 i = 0; i < count[(size_t)v]; ++i) {
                const u32 e = index[(size_t)(v * k + i)];
                neighbour.push_back(ea[e] == v ? eb[e] : ea[e]);
                hit_text.push_back(text[e]);
            }
        ksp::write_topk_file(out_path && *out_path ? std::string(out_path) : prefix + "_kSpider_topk_" + dt + ".tsv", dt, name_of, count, neighbour, hit_text);
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: top " << k << " of " << n << " records: " << neighbour.size() << " hits written; nodes selected by wave / workgroup / stream kernel: "
                      << g_trace.wave << " / " << g_trace.workgroup << " / " << g_trace.stream << std::endl;
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}
