// Query mode: new sketches against a database that stays in HBM, without the N x N join.  Every database hash
// is read exactly once per tile of queries and looked up in a small sorted table built from the queries; no partition, no
// block lists, no tiles of source pairs.
//
// Numbering.  Database sources are 0 .. n_db - 1, queries n_db .. n_db + n_q - 1.  An edge is a ksp_edge with
//   source_1 < source_2 in that numbering and shared > 0: KSP_QUERY_CROSS gives the database x query pairs,
//   KSP_QUERY_CROSS_AND_SELF also every query x query pair once.
//
//   table    per tile of at most KSP_QUERY_TILE consecutive queries: the collision-free sorted table with its directory
//            (query_table.hip.h, shared with gather.hip).
//   probe    the probe sources are the database sources, followed in mode 1 by the queries.  A source's pair counters are u32
//            in LDS, one per query of the tile.  k_query_probe<true>: one wave per source with wave-private counters, for runs
//            below KSP_QUERY_LONG_RUN entries; k_query_probe<false>: one 256-thread workgroup per source for the others.  A lane
//            looks its hash up and on a hit adds 1 to the counter of every holder; a holder whose add returned 0 goes to a
//            touched list in LDS.  In mode 1 a probing query i skips the holders j <= i.  Emission walks the touched list (or,
//            when it overflowed, all counters of the tile), reads and clears the counters and appends the edges: one ballot,
//            one returning add on a 64-bit cursor per wave, stores guarded by the capacity.
// A run is never split over workgroups (two halves would emit the same pair twice): a very long source is one workgroup's loop.
// Every loop is bounded by a size the host computed; no workgroup waits on another.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"
#include "query_table.hip.h"

namespace {

constexpr u32 kTileMax = KSP_QUERY_TILE_MAX;   // queries per tile: 8 KiB of counters per group
constexpr u32 kListMax = KSP_QUERY_LIST_MAX;   // touched-list entries per group: 2 KiB
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// the wave kernel holds four groups: 4 x (8 + 2) KiB + 16 bytes; four of its workgroups fit the 160 KiB of a CU
static_assert(2 * (kWaves * (kTileMax + kListMax) * 4 + 64) <= 160 * 1024, "two workgroups per CU");
static_assert(kWaves * (kTileMax + kListMax) * 4 + 64 <= 64 * 1024, "static LDS of one workgroup");

// what a probe kernel reads and writes besides the table
struct QProbe {
    const u64 *db_keys, *db_off, *q_keys, *q_off;
    u32 n_db;
    const u32* list;   // the probe sources of this kernel, in the common numbering
    u32 n_list;
    u32 list_cap;      // touched-list capacity, 1 .. kListMax
    ksp_edge* edges;
    u64 capacity;
    unsigned long long* cursor;      // edges appended so far, the ones that found no room included
    unsigned long long* overflows;   // sources whose touched list overflowed
};

// One group per probe source: a wave (kWave, four groups per workgroup) or the whole workgroup.  cnt[t]: the keys the source
// shares with query t of the tile; list[0 .. min(*n, cap)): the queries whose counter left 0.
template <bool kWave>
__global__ __launch_bounds__(kThreads) void k_query_probe(const QTable T, const QProbe P) {
    constexpr u32 kGroups = kWave ? kWaves : 1;
    constexpr u32 kLanes = kWave ? 64 : kThreads;
    __shared__ u32 s_cnt[kGroups][kTileMax];
    __shared__ u32 s_list[kGroups][kListMax];
    __shared__ u32 s_n[kGroups];
    const u32 g = kWave ? threadIdx.x >> 6 : 0, t = kWave ? threadIdx.x & 63 : threadIdx.x, lane = threadIdx.x & 63;
    u32* const cnt = s_cnt[g];
    u32* const list = s_list[g];
    u32* const n = &s_n[g];
    for (u32 j = t; j < T.nq; j += kLanes) cnt[j] = 0;
    if (t == 0) *n = 0;
    query_group_sync<kWave>();
    const u64 first = kWave ? (u64)blockIdx.x * kWaves + g : blockIdx.x, stride = kWave ? (u64)gridDim.x * kWaves : gridDim.x;
    for (u64 i = first; i < P.n_list; i += stride) {
        const u32 p = P.list[i];
        const bool is_q = p >= P.n_db;
        const u32 qi = is_q ? p - P.n_db : 0;
        if (is_q && (u64)qi + 1 >= (u64)T.q0 + T.nq) continue;   // (the same for the whole group) no holder of this tile is above query qi
        const u32 min_tag = is_q && qi >= T.q0 ? qi - T.q0 + 1 : 0;   // mode 1: a probing query skips the holders j <= i
        const u64* const keys = is_q ? P.q_keys : P.db_keys;
        const u64 o0 = is_q ? P.q_off[qi] : P.db_off[p], o1 = is_q ? P.q_off[qi + 1] : P.db_off[p + 1];
        for (u64 e = o0 + t; e < o1; e += (u64)kLanes * kProbeKeys) {
            u64 k[kProbeKeys];
            bool live[kProbeKeys];
            u32 at[kProbeKeys];
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x) {
                const u64 ex = e + (u64)x * kLanes;
                live[x] = ex < o1;
                k[x] = live[x] ? keys[ex] : 0;
            }
            query_lookup(T, k, live, at);
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x) {
                if (!live[x]) continue;
                const u32 h1 = T.toff[at[x] + 1];
                for (u32 h = T.toff[at[x]]; h < h1; ++h) {
                    const u32 tag = T.tq[h];
                    if (tag < min_tag || tag >= T.nq) continue;   // (a tag is below nq by construction)
                    if (atomicAdd(&cnt[tag], 1u) == 0) {
                        const u32 pos = atomicAdd(n, 1u);
                        if (pos < P.list_cap) list[pos] = tag;
                    }
                }
            }
        }
        query_group_sync<kWave>();
        const u32 touched = *n;
        query_group_sync<kWave>();
        if (t == 0) *n = 0;   // (the next source's adds come behind the sync at the end of the emission)
        const bool over = touched > P.list_cap;   // the list lost entries: one scan over all counters replaces it
        if (over && t == 0) atomicAdd(P.overflows, 1ull);
        const u32 count = over ? T.nq : touched;
        for (u32 base = 0; base < count; base += kLanes) {   // (the same trips for every lane of the group)
            const u32 j = base + t;
            u32 tag = 0, c = 0;
            if (j < count) {
                tag = over ? j : list[j];
                c = cnt[tag];
                if (c) cnt[tag] = 0;
            }
            const unsigned long long have = __ballot(c != 0);
            if (!have) continue;   // (the whole wave)
            unsigned long long at = 0;
            if (lane == (u32)__ffsll((long long)have) - 1) at = atomicAdd(P.cursor, (unsigned long long)__popcll(have));
            const int src = __ffsll((long long)have) - 1;
            const u32 at_lo = (u32)__shfl((int)(u32)at, src), at_hi = (u32)__shfl((int)(u32)(at >> 32), src);
            const u64 slot = (((u64)at_hi << 32) | at_lo) + (u64)__popcll(have & ((1ull << lane) - 1));
            if (c && slot < P.capacity) P.edges[slot] = ksp_edge{p, P.n_db + T.q0 + tag, (u64)c};
        }
        query_group_sync<kWave>();
    }
}

struct EdgeBefore {
    __host__ __device__ bool operator()(const ksp_edge& a, const ksp_edge& b) const {
        return a.source_1 != b.source_1 ? a.source_1 < b.source_1 : a.source_2 < b.source_2;
    }
};

// what both entry points refuse before anything is allocated
int check_query_args(const char* who, const void* db_keys, const u64* db_off, const u32 n_db, const void* q_keys, const u64* q_off, const u32 n_q, const int mode,
                     const void* n_edges) {
    if (!db_keys || !db_off || !q_keys || !q_off || !n_edges) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_db == 0 || n_q == 0) { ksp::set_error(std::string(who) + ": no database source or no query"); return KSP_E_ARG; }
    if (mode != KSP_QUERY_CROSS && mode != KSP_QUERY_CROSS_AND_SELF) {
        ksp::set_error(std::string(who) + ": mode is KSP_QUERY_CROSS (0) or KSP_QUERY_CROSS_AND_SELF (1)");
        return KSP_E_ARG;
    }
    if ((u64)n_db + n_q > 0xFFFFFFFEull) { ksp::set_error(std::string(who) + ": more than 2^32 - 2 sources"); return KSP_E_LIMIT; }   // (from the counts alone)
    if (const int rc = check_offsets(who, "database", db_off, n_db)) return rc;
    return check_offsets(who, "query", q_off, n_q);
}

// The query on the CURRENT device; the arguments have passed check_query_args.
int query_on_device(const char* who, const u64* d_db_keys, const u64* h_db_off, const u32 n_db, const u64* d_q_keys, const u64* h_q_off, const u32 n_q, const int mode,
                    ksp_edge* d_edges, const u64 capacity, u64* n_edges, ksp_query_stats* stats) {
    int rc = KSP_OK;
    ksp_query_stats S;
    std::memset(&S, 0, sizeof S);
    u64 tile = 0, long_run = 0, list_cap = 0;
    ksp::WorkgroupCap G;
    if ((rc = env_number(who, "KSP_QUERY_TILE", kTileMax, 1, kTileMax, &tile)) || (rc = env_number(who, "KSP_QUERY_LONG_RUN", KSP_QUERY_LONG_RUN, 1, ~0ull, &long_run)) ||
        (rc = env_number(who, "KSP_QUERY_LIST", kListMax, 1, kListMax, &list_cap)))
        return rc;
    // the tiles and the largest of them
    u32 n_tiles = 0;
    u64 e_max = 0;
    if ((rc = query_tiles(who, h_q_off, n_q, tile, &n_tiles, &e_max))) return rc;
    if ((rc = ksp::workgroup_cap("KSP_QUERY_MAX_WORKGROUPS", who, G))) return rc;
    // the probe sources by run length: the database's, then in mode 1 the queries (the last query has no query above it)
    std::vector<u32> probes[2];   // [0] short, [1] long
    query_split_sources(h_db_off, n_db, long_run, 0, probes);
    if (mode == KSP_QUERY_CROSS_AND_SELF) query_split_sources(h_q_off, n_q - 1, long_run, n_db, probes);
    S.n_db = n_db; S.n_q = n_q; S.db_entries = h_db_off[n_db]; S.q_entries = h_q_off[n_q];
    S.short_sources = probes[0].size(); S.long_sources = probes[1].size();
    S.tile = (u32)tile; S.long_run = long_run; S.list_capacity = (u32)list_cap;

    ksp::DeviceArena A;
    ksp::Events<3> ev;
    QTableBufs B;
    B.e_max = e_max;
    if ((rc = query_table_scratch(e_max, &B.tb))) return rc;
    B.tb = std::max<size_t>(B.tb, 8);
    // ---- everything the call holds, sized and checked first: 8 per source (offsets), 4 per probe source, and per entry of the
    // largest tile 40 (tag 4, sorted key 8 and tag 4, scan 8, table key 8, holder range 4, holder 4), the directory, the scratch
    if ((rc = ksp::device_fits(who, 8ull * ((u64)n_db + n_q + 2) + 4ull * (probes[0].size() + probes[1].size()) + B.bytes() + B.tb + 64,
                               "8 per source, 4 per probe source, 40 per entry of the largest query tile, its directory, the sort's scratch")))
        return rc;
    u64 *d_db_off = nullptr, *d_q_off = nullptr;
    u32* d_list[2] = {nullptr, nullptr};
    unsigned long long* d_count = nullptr;   // [0] the cursor, [1] the list overflows
    if ((rc = query_upload_front(A, h_db_off, n_db, h_q_off, n_q, probes, &d_db_off, &d_q_off, d_list)) || (rc = A.alloc(&d_count, 2))) return rc;
    if (e_max && ((rc = query_table_alloc(A, B)) || (rc = A.alloc_bytes(&B.tmp, B.tb)))) return rc;
    KSP_HIP(hipMemset(d_count, 0, 16));
    if ((rc = ev.create())) return rc;

    for (u32 t = 0; t < n_tiles; ++t) {
        const u32 q0 = (u32)((u64)t * tile), nq = (u32)(std::min<u64>((u64)q0 + tile, n_q) - q0);
        const u64 e0 = h_q_off[q0];
        const u32 E = (u32)(h_q_off[q0 + nq] - e0);
        if (E == 0) continue;   // a tile of empty queries shares nothing
        // ---- the table
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        QTable T;
        u32 U = 0, H = 0;
        if ((rc = query_table_build(who, G, B, d_q_keys, d_q_off, q0, nq, e0, E, &T, &U, &H))) return rc;
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        // ---- the probe: every probe source against this tile
        QProbe P{d_db_keys, d_db_off, d_q_keys, d_q_off, n_db, nullptr, 0, (u32)list_cap, d_edges, d_edges ? capacity : 0, &d_count[0], &d_count[1]};
        if (!probes[0].empty()) {
            P.list = d_list[0]; P.n_list = (u32)probes[0].size();
            hipLaunchKernelGGL(k_query_probe<true>, dim3(G.grid_of(((u64)P.n_list + kWaves - 1) / kWaves)), dim3(kThreads), 0, nullptr, T, P);
        }
        if (!probes[1].empty()) {
            P.list = d_list[1]; P.n_list = (u32)probes[1].size();
            hipLaunchKernelGGL(k_query_probe<false>, dim3(G.grid_of(P.n_list)), dim3(kThreads), 0, nullptr, T, P);
        }
        KSP_HIP(hipGetLastError());
        KSP_HIP(hipEventRecord(ev[2], nullptr));
        KSP_HIP(hipEventSynchronize(ev[2]));
        float ms_t = 0, ms_p = 0;
        KSP_HIP(hipEventElapsedTime(&ms_t, ev[0], ev[1]));
        KSP_HIP(hipEventElapsedTime(&ms_p, ev[1], ev[2]));
        S.ms_table += ms_t; S.ms_probe += ms_p;
        S.table_keys += U; S.table_holders += H; ++S.passes;
    }
    unsigned long long h_count[2] = {0, 0};
    KSP_HIP(hipMemcpy(h_count, d_count, 16, hipMemcpyDeviceToHost));
    S.edges = h_count[0]; S.list_overflows = h_count[1];
    *n_edges = h_count[0];
    if (stats) *stats = S;
    if (h_count[0] > capacity) {
        ksp::set_error(std::string(who) + ": " + std::to_string(h_count[0]) + " edges, room for " + std::to_string(capacity));
        return KSP_E_OVERFLOW;
    }
    return KSP_OK;
}

}  // namespace

extern "C" int ksp_query_directory(uint64_t max_key, uint64_t n_keys, int* bits, int* shift) {
    if (!bits || !shift) { ksp::set_error("ksp_query_directory: NULL argument"); return KSP_E_ARG; }
    int key_bits = 0;
    while (key_bits < 64 && (max_key >> key_bits)) ++key_bits;   // the significant bits of the largest key
    int b = 0;
    while (b < KSP_QUERY_DIR_BITS_MAX && (4ull << b) < n_keys) ++b;   // about four keys per bucket of a uniform table
    b = std::min(std::max(b, 1), std::max(key_bits, 1));   // (at least one bit: the shift stays below 64)
    *bits = key_bits ? b : 0;
    *shift = key_bits ? key_bits - b : 0;
    return KSP_OK;
}

extern "C" int ksp_debug_copy_times(int device, uint64_t bytes, int reps, float* ms) {
    const char* who = "ksp_debug_copy_times";
    if (!ms || reps < 1 || !bytes) { ksp::set_error(std::string(who) + ": bad argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::Events<2> ev;
    void *src = nullptr, *dst = nullptr;
    if ((rc = ksp::device_fits(who, 2 * bytes, "two buffers")) || (rc = A.alloc_bytes(&src, (size_t)bytes)) || (rc = A.alloc_bytes(&dst, (size_t)bytes))) return rc;
    KSP_HIP(hipMemset(src, 1, (size_t)bytes));
    if ((rc = ev.create())) return rc;
    for (int r = 0; r < reps; ++r) {
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        KSP_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, nullptr));
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        KSP_HIP(hipEventSynchronize(ev[1]));
        KSP_HIP(hipEventElapsedTime(&ms[r], ev[0], ev[1]));
    }
    return KSP_OK;
}

extern "C" int ksp_query_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys,
                                const uint64_t* h_q_offsets, uint32_t n_q, int mode, ksp_edge* d_edges, uint64_t capacity, uint64_t* n_edges, ksp_query_stats* stats) {
    const char* who = "ksp_query_device";
    if (const int rc = check_query_args(who, d_db_keys, h_db_offsets, n_db, d_q_keys, h_q_offsets, n_q, mode, n_edges)) return rc;
    if (!d_edges && capacity) { ksp::set_error(std::string(who) + ": d_edges is NULL but capacity is not 0"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return query_on_device(who, d_db_keys, h_db_offsets, n_db, d_q_keys, h_q_offsets, n_q, mode, d_edges, capacity, n_edges, stats);
}

extern "C" int ksp_query_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint64_t* q_offsets, uint32_t n_q,
                              int mode, int device, ksp_edge** edges, uint64_t* n_edges, ksp_query_stats* stats) {
    const char* who = "ksp_query_host";
    if (!edges) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (const int rc = check_query_args(who, db_keys, db_offsets, n_db, q_keys, q_offsets, n_q, mode, n_edges)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::Events<2> ev;
    const u64 n_dbk = db_offsets[n_db], n_qk = q_offsets[n_q];
    u64 *d_db = nullptr, *d_q = nullptr, found = 0;
    ksp_edge* d_edges = nullptr;
    ksp_query_stats S;
    // a first guess that a few hits per query satisfy; the call reports the exact size when it does not
    u64 capacity = std::max<u64>(4096, 8ull * ((u64)n_db + n_q));
    if ((rc = ksp::device_fits(who, 8ull * (n_dbk + n_qk + 2) + 16ull * capacity, "the keys of both sides and the first edge buffer"))) return rc;
    if ((rc = query_upload_keys(A, db_keys, n_dbk, q_keys, n_qk, &d_db, &d_q)) || (rc = A.alloc(&d_edges, (size_t)capacity))) return rc;
    rc = query_on_device(who, d_db, db_offsets, n_db, d_q, q_offsets, n_q, mode, d_edges, capacity, &found, &S);
    if (rc == KSP_E_OVERFLOW) {   // once more, at the exact size
        KSP_HIP(A.release(d_edges));
        d_edges = nullptr;
        capacity = found;
        if ((rc = ksp::device_fits(who, 16ull * capacity, "the edges"))) return rc;
        if ((rc = A.alloc(&d_edges, (size_t)capacity))) return rc;
        rc = query_on_device(who, d_db, db_offsets, n_db, d_q, q_offsets, n_q, mode, d_edges, capacity, &found, &S);
    }
    if (rc != KSP_OK) return rc;
    if ((rc = ev.create())) return rc;
    std::unique_ptr<ksp_edge, decltype(&std::free)> h_edges((ksp_edge*)std::malloc((size_t)std::max<u64>(found, 1) * sizeof(ksp_edge)), &std::free);
    if (!h_edges) { ksp::set_error(std::string(who) + ": out of host memory"); return KSP_E_LIMIT; }
    if (found) {
        ksp_edge* d_sorted = nullptr;
        void* tmp = nullptr;
        size_t tb = 0;
        KSP_HIP(rocprim::merge_sort(nullptr, tb, (const ksp_edge*)d_edges, d_sorted, (size_t)found, EdgeBefore(), (hipStream_t) nullptr));
        tb = std::max<size_t>(tb, 8);
        if ((rc = ksp::device_fits(who, 16ull * found + tb, "the sorted edges and the sort's scratch"))) return rc;
        if ((rc = A.alloc(&d_sorted, (size_t)found)) || (rc = A.alloc_bytes(&tmp, tb))) return rc;
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        KSP_HIP(rocprim::merge_sort(tmp, tb, (const ksp_edge*)d_edges, d_sorted, (size_t)found, EdgeBefore(), (hipStream_t) nullptr));
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        KSP_HIP(hipMemcpy(h_edges.get(), d_sorted, (size_t)found * sizeof(ksp_edge), hipMemcpyDeviceToHost));
        KSP_HIP(hipEventElapsedTime(&S.ms_sort, ev[0], ev[1]));
    }
    *edges = h_edges.release();
    *n_edges = found;
    if (stats) *stats = S;
    return KSP_OK;
}
