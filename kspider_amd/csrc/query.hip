// Query mode: new sketches against a database that stays in HBM, without the N x N join.  Every database hash
// is read exactly once per tile of queries and looked up in a small sorted table built from the queries; no partition, no
// block lists, no tiles of source pairs.
//
// Numbering.  Database sources are 0 .. n_db - 1, queries n_db .. n_db + n_q - 1.  An edge is a ksp_edge with
//   source_1 < source_2 in that numbering and shared > 0: KSP_QUERY_CROSS gives the database x query pairs,
//   KSP_QUERY_CROSS_AND_SELF also every query x query pair once.
//
//   table    per tile of at most KSP_QUERY_TILE consecutive queries: every query entry tagged with its query index inside the
//            tile (k_query_tag), (key, tag) sorted by key with rocPRIM's radix sort (stable: the tags of a key ascend), adjacent
//            duplicates dropped by one scan of packed (head, kept) flags and k_query_compact.  Result: the distinct keys tk[U],
//            the holder ranges toff[U + 1] and the holders tq[].  First level: dir[b] = the first index whose key >> shift is
//            >= b (k_query_dir; bits and shift: ksp_query_directory), then a binary search inside the bucket.  A probe key above
//            tk[U - 1] misses without a memory access.  No hash function, no compare-and-swap build, no collisions.
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
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kTileMax = KSP_QUERY_TILE_MAX;   // queries per tile: 8 KiB of counters per group
constexpr u32 kListMax = KSP_QUERY_LIST_MAX;   // touched-list entries per group: 2 KiB
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
// the wave kernel holds four groups: 4 x (8 + 2) KiB + 16 bytes; four of its workgroups fit the 160 KiB of a CU
static_assert(2 * (kWaves * (kTileMax + kListMax) * 4 + 64) <= 160 * 1024, "two workgroups per CU");
static_assert(kWaves * (kTileMax + kListMax) * 4 + 64 <= 64 * 1024, "static LDS of one workgroup");

// one tile's table (device pointers), by value into the probe kernels
struct QTable {
    const u64* tk;     // U distinct keys, ascending
    const u32* toff;   // U + 1: the holders of key u are tq[toff[u] .. toff[u + 1])
    const u32* tq;     // holders: query indices inside the tile, ascending within a key
    const u32* dir;    // n_buckets + 1: dir[b] = the first index whose key >> shift is >= b
    u64 max_key;       // tk[U - 1]
    int shift;
    u32 q0, nq;        // the tile's queries: q0 .. q0 + nq - 1 (indices among the queries)
};

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

// tag[i] = the query (inside the tile) that holds entry e0 + i: the last offset that is <= the entry
__global__ void k_query_tag(const u64* __restrict__ q_off, const u32 q0, const u32 nq, const u64 e0, const u32 E, u32* __restrict__ tag) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (u64)gridDim.x * blockDim.x) {
        const u64 e = e0 + i;
        u32 lo = 0, hi = nq;   // the answer is in [lo, hi): q_off[q0 + lo] <= e < q_off[q0 + hi]
        while (hi - lo > 1) {
            const u32 mid = lo + (hi - lo) / 2;
            if (q_off[q0 + mid] <= e) lo = mid; else hi = mid;
        }
        tag[i] = lo;
    }
}

// (head << 32) | kept of sorted entry i: head = the first entry of its key, kept = head or another holder than the entry before
struct QFlags {
    const u64* key;
    const u32* tag;
    u32 E;
    __host__ __device__ u64 operator()(const u32 i) const {
        if (i >= E) return 0;
        const bool head = i == 0 || key[i] != key[i - 1];
        const bool kept = head || tag[i] != tag[i - 1];
        return ((u64)head << 32) | (u64)kept;
    }
};

// scan[i] = (heads << 32) | kept before entry i (E + 1 values: the last is the totals U and H)
__global__ void k_query_compact(const u64* __restrict__ key, const u32* __restrict__ tag, const u64* __restrict__ scan, const u32 E, u64* __restrict__ tk,
                                u32* __restrict__ toff, u32* __restrict__ tq) {
    const QFlags flags{key, tag, E};
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < E; i += (u64)gridDim.x * blockDim.x) {
        const u64 f = flags((u32)i), s = scan[i];
        const u32 h = (u32)s, u = (u32)(s >> 32);
        if (f & 1) tq[h] = tag[i];
        if (f >> 32) { tk[u] = key[i]; toff[u] = h; }
        if (i == 0) toff[(u32)(scan[E] >> 32)] = (u32)scan[E];
    }
}

// dir[b] = the first index whose key is >= b << shift, b = 0 .. n_buckets (the last: U)
__global__ void k_query_dir(const u64* __restrict__ tk, const u32 U, const int shift, const u32 n_buckets, u32* __restrict__ dir) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b <= n_buckets; b += (u64)gridDim.x * blockDim.x) {
        u32 lo = 0, hi = U;
        if (b == n_buckets) lo = U;
        const u64 first = b << shift;
        while (lo < hi) {
            const u32 mid = lo + (hi - lo) / 2;
            if (tk[mid] < first) lo = mid + 1; else hi = mid;
        }
        dir[b] = lo;
    }
}

// A lane looks kProbeKeys keys up at a time, step by step for all of them, so that the loads of a step — the keys, the bucket
// bounds, a halving of every search, the final compare — are in flight together: a look-up is a chain of dependent loads from
// L2 / Infinity Cache, and one chain at a time leaves the lane waiting on each (measured: DESIGN.md 7n).
constexpr int kProbeKeys = 4;

// at[x] = the index of k[x] in the table for every x whose live[x] stays set (a key above the largest misses without a load)
__device__ inline void query_lookup(const QTable& T, const u64 (&k)[kProbeKeys], bool (&live)[kProbeKeys], u32 (&at)[kProbeKeys]) {
    u32 lo[kProbeKeys], hi[kProbeKeys], end[kProbeKeys];
#pragma unroll
    for (int x = 0; x < kProbeKeys; ++x) {
        live[x] = live[x] && k[x] <= T.max_key;
        const u32 b = live[x] ? (u32)(k[x] >> T.shift) : 0;
        lo[x] = live[x] ? T.dir[b] : 0;
        end[x] = hi[x] = live[x] ? T.dir[b + 1] : 0;
    }
    bool more = true;
    while (more) {   // (a bucket of a uniform table holds about four keys: two or three rounds)
        u32 mid[kProbeKeys];
        u64 v[kProbeKeys];
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            mid[x] = lo[x] + (hi[x] - lo[x]) / 2;
            v[x] = lo[x] < hi[x] ? T.tk[mid[x]] : 0;
        }
        more = false;
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            if (lo[x] >= hi[x]) continue;
            if (v[x] < k[x]) lo[x] = mid[x] + 1; else hi[x] = mid[x];
            more |= lo[x] < hi[x];
        }
    }
    u64 found[kProbeKeys];
#pragma unroll
    for (int x = 0; x < kProbeKeys; ++x) found[x] = lo[x] < end[x] ? T.tk[lo[x]] : 0;
#pragma unroll
    for (int x = 0; x < kProbeKeys; ++x) {
        live[x] = lo[x] < end[x] && found[x] == k[x];   // (end is 0 for a key that was not live)
        at[x] = lo[x];
    }
}

// everything the group's lanes wrote to its LDS is visible to all of them behind this
template <bool kWave>
__device__ inline void query_group_sync() {
    if (kWave) {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    } else {
        __syncthreads();
    }
}

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

// $name as a number in [lo, hi], or `fallback` when it is unset or empty
int env_number(const char* who, const char* name, const u64 fallback, const u64 lo, const u64 hi, u64* out) {
    const char* s = std::getenv(name);
    *out = fallback;
    if (!s || !*s) return KSP_OK;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(s, &end, 10);
    if (end == s || *end || *s == '-' || v < lo || v > hi) {
        ksp::set_error(std::string(who) + ": " + name + " is a number from " + std::to_string(lo) + " to " + std::to_string(hi));
        return KSP_E_ARG;
    }
    *out = v;
    return KSP_OK;
}

int check_offsets(const char* who, const char* what, const u64* off, const u32 n) {
    if (off[0] != 0) { ksp::set_error(std::string(who) + ": the " + what + " offsets do not start at 0"); return KSP_E_ARG; }
    for (u32 s = 0; s < n; ++s)
        if (off[s + 1] < off[s]) { ksp::set_error(std::string(who) + ": the " + what + " offsets decrease at source " + std::to_string(s)); return KSP_E_ARG; }
    return KSP_OK;
}

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
    const u32 n_tiles = (u32)(((u64)n_q + tile - 1) / tile);
    u64 e_max = 0;
    for (u32 t = 0; t < n_tiles; ++t) {
        const u64 q0 = (u64)t * tile, q1 = std::min<u64>(q0 + tile, n_q), E = h_q_off[q1] - h_q_off[q0];
        if (E >= (1ull << 31)) { ksp::set_error(std::string(who) + ": a query tile of 2^31 entries or more (lower KSP_QUERY_TILE)"); return KSP_E_LIMIT; }
        e_max = std::max(e_max, E);
    }
    if ((rc = ksp::workgroup_cap("KSP_QUERY_MAX_WORKGROUPS", who, G))) return rc;
    // the probe sources by run length; a source without entries shares nothing
    std::vector<u32> probes[2];   // [0] short, [1] long
    for (u32 p = 0; p < n_db; ++p)
        if (const u64 len = h_db_off[p + 1] - h_db_off[p]) probes[len >= long_run].push_back(p);
    if (mode == KSP_QUERY_CROSS_AND_SELF)
        for (u32 i = 0; i + 1 < n_q; ++i)   // (the last query has no query above it)
            if (const u64 len = h_q_off[i + 1] - h_q_off[i]) probes[len >= long_run].push_back(n_db + i);
    S.n_db = n_db; S.n_q = n_q; S.db_entries = h_db_off[n_db]; S.q_entries = h_q_off[n_q];
    S.short_sources = probes[0].size(); S.long_sources = probes[1].size();
    S.tile = (u32)tile; S.long_run = long_run; S.list_capacity = (u32)list_cap;

    ksp::DeviceArena A;
    u64 *d_db_off = nullptr, *d_q_off = nullptr, *skey = nullptr, *scan = nullptr, *tk = nullptr;
    u32 *d_list[2] = {nullptr, nullptr}, *tag = nullptr, *stag = nullptr, *toff = nullptr, *tq = nullptr, *dir = nullptr;
    unsigned long long* d_count = nullptr;   // [0] the cursor, [1] the list overflows
    void* tmp = nullptr;
    size_t tb_sort = 0, tb_scan = 0, tb = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    unsigned long long h_count[2] = {0, 0};
    const u64 dir_max = (1ull << KSP_QUERY_DIR_BITS_MAX) + 1;
    const auto flags_of = [](const u64* k, const u32* t, const u32 E) {
        return rocprim::make_transform_iterator(rocprim::counting_iterator<u32>(0), QFlags{k, t, E});
    };
    if (e_max) {
        KSP_TRY_HIP(rocprim::radix_sort_pairs(nullptr, tb_sort, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)e_max, 0, 64, (hipStream_t) nullptr));
        KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, flags_of(nullptr, nullptr, 0), (u64*)nullptr, (u64)0, (size_t)e_max + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
    }
    tb = std::max<size_t>(std::max(tb_sort, tb_scan), 8);
    // ---- everything the call holds, sized and checked first: 8 per source (offsets), 4 per probe source, and per entry of the
    // largest tile 40 (tag 4, sorted key 8 and tag 4, scan 8, table key 8, holder range 4, holder 4), the directory, the scratch
    if ((rc = ksp::device_fits(who, 8ull * ((u64)n_db + n_q + 2) + 4ull * (probes[0].size() + probes[1].size()) + 40ull * (e_max + 1) + 4 * std::min<u64>(dir_max, e_max + 2) + tb + 64,
                               "8 per source, 4 per probe source, 40 per entry of the largest query tile, its directory, the sort's scratch")))
        return rc;
    if ((rc = A.alloc(&d_db_off, (size_t)n_db + 1)) || (rc = A.alloc(&d_q_off, (size_t)n_q + 1)) || (rc = A.alloc(&d_count, 2))) return rc;
    for (int c = 0; c < 2; ++c)
        if (!probes[c].empty() && (rc = A.alloc(&d_list[c], probes[c].size()))) return rc;
    if (e_max) {
        if ((rc = A.alloc(&tag, (size_t)e_max)) || (rc = A.alloc(&skey, (size_t)e_max)) || (rc = A.alloc(&stag, (size_t)e_max)) || (rc = A.alloc(&scan, (size_t)e_max + 1)) ||
            (rc = A.alloc(&tk, (size_t)e_max)) || (rc = A.alloc(&toff, (size_t)e_max + 1)) || (rc = A.alloc(&tq, (size_t)e_max)) ||
            (rc = A.alloc(&dir, (size_t)std::min<u64>(dir_max, e_max + 2))) || (rc = A.alloc_bytes(&tmp, tb)))
            return rc;
    }
    KSP_TRY_HIP(hipMemcpy(d_db_off, h_db_off, ((size_t)n_db + 1) * 8, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemcpy(d_q_off, h_q_off, ((size_t)n_q + 1) * 8, hipMemcpyHostToDevice));
    for (int c = 0; c < 2; ++c)
        if (!probes[c].empty()) KSP_TRY_HIP(hipMemcpy(d_list[c], probes[c].data(), probes[c].size() * 4, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemset(d_count, 0, 16));
    for (hipEvent_t& e : ev) KSP_TRY_HIP(hipEventCreate(&e));

    for (u32 t = 0; t < n_tiles; ++t) {
        const u32 q0 = (u32)((u64)t * tile), nq = (u32)(std::min<u64>((u64)q0 + tile, n_q) - q0);
        const u64 e0 = h_q_off[q0];
        const u32 E = (u32)(h_q_off[q0 + nq] - e0);
        if (E == 0) continue;   // a tile of empty queries shares nothing
        // ---- the table
        KSP_TRY_HIP(hipEventRecord(ev[0], nullptr));
        const unsigned ge = G.grid_of(((u64)E + 255) / 256);
        hipLaunchKernelGGL(k_query_tag, dim3(ge), dim3(256), 0, nullptr, (const u64*)d_q_off, q0, nq, e0, E, tag);
        KSP_TRY_HIP(hipGetLastError());
        {
            size_t b = 0, b2 = 0;   // (the scratch was sized for the largest tile: a smaller one must not ask for more)
            KSP_TRY_HIP(rocprim::radix_sort_pairs(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)E, 0, 64, (hipStream_t) nullptr));
            KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, b2, flags_of(nullptr, nullptr, 0), (u64*)nullptr, (u64)0, (size_t)E + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
            if (std::max(b, b2) > tb) { ksp::set_error(std::string(who) + ": a smaller tile asks for more scratch than the largest"); rc = KSP_E_HIP; goto done; }
            b = tb;
            KSP_TRY_HIP(rocprim::radix_sort_pairs(tmp, b, d_q_keys + e0, skey, (const u32*)tag, stag, (size_t)E, 0, 64, (hipStream_t) nullptr));
            b = tb;
            KSP_TRY_HIP(rocprim::exclusive_scan(tmp, b, flags_of(skey, stag, E), scan, (u64)0, (size_t)E + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        }
        u64 totals = 0, max_key = 0;
        KSP_TRY_HIP(hipMemcpy(&totals, scan + E, 8, hipMemcpyDeviceToHost));
        const u32 U = (u32)(totals >> 32), H = (u32)totals;
        if (U == 0 || U > E || H < U || H > E) { ksp::set_error(std::string(who) + ": the query table lost its keys"); rc = KSP_E_HIP; goto done; }
        hipLaunchKernelGGL(k_query_compact, dim3(ge), dim3(256), 0, nullptr, (const u64*)skey, (const u32*)stag, (const u64*)scan, E, tk, toff, tq);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipMemcpy(&max_key, tk + (U - 1), 8, hipMemcpyDeviceToHost));
        int bits = 0, shift = 0;
        (void)ksp_query_directory(max_key, U, &bits, &shift);
        const u32 n_buckets = 1u << bits;
        if ((u64)n_buckets + 1 > std::min<u64>(dir_max, (u64)e_max + 2)) { ksp::set_error(std::string(who) + ": the directory outgrew its buffer"); rc = KSP_E_HIP; goto done; }
        hipLaunchKernelGGL(k_query_dir, dim3(G.grid_of(((u64)n_buckets + 256) / 256)), dim3(256), 0, nullptr, (const u64*)tk, U, shift, n_buckets, dir);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipEventRecord(ev[1], nullptr));
        // ---- the probe: every probe source against this tile
        {
            const QTable T{tk, toff, tq, dir, max_key, shift, q0, nq};
            QProbe P{d_db_keys, d_db_off, d_q_keys, d_q_off, n_db, nullptr, 0, (u32)list_cap, d_edges, d_edges ? capacity : 0, &d_count[0], &d_count[1]};
            if (!probes[0].empty()) {
                P.list = d_list[0]; P.n_list = (u32)probes[0].size();
                hipLaunchKernelGGL(k_query_probe<true>, dim3(G.grid_of(((u64)P.n_list + kWaves - 1) / kWaves)), dim3(kThreads), 0, nullptr, T, P);
            }
            if (!probes[1].empty()) {
                P.list = d_list[1]; P.n_list = (u32)probes[1].size();
                hipLaunchKernelGGL(k_query_probe<false>, dim3(G.grid_of(P.n_list)), dim3(kThreads), 0, nullptr, T, P);
            }
            KSP_TRY_HIP(hipGetLastError());
        }
        KSP_TRY_HIP(hipEventRecord(ev[2], nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev[2]));
        float ms_t = 0, ms_p = 0;
        KSP_TRY_HIP(hipEventElapsedTime(&ms_t, ev[0], ev[1]));
        KSP_TRY_HIP(hipEventElapsedTime(&ms_p, ev[1], ev[2]));
        S.ms_table += ms_t; S.ms_probe += ms_p;
        S.table_keys += U; S.table_holders += H; ++S.passes;
    }
    KSP_TRY_HIP(hipMemcpy(h_count, d_count, 16, hipMemcpyDeviceToHost));
    S.edges = h_count[0]; S.list_overflows = h_count[1];
    *n_edges = h_count[0];
    if (stats) *stats = S;
    if (h_count[0] > capacity) {
        ksp::set_error(std::string(who) + ": " + std::to_string(h_count[0]) + " edges, room for " + std::to_string(capacity));
        rc = KSP_E_OVERFLOW;
    }
done:
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
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
    void *src = nullptr, *dst = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if ((rc = ksp::device_fits(who, 2 * bytes, "two buffers")) || (rc = A.alloc_bytes(&src, (size_t)bytes)) || (rc = A.alloc_bytes(&dst, (size_t)bytes))) return rc;
    KSP_TRY_HIP(hipMemset(src, 1, (size_t)bytes));
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        KSP_TRY_HIP(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, nullptr));
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
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
    const u64 n_dbk = db_offsets[n_db], n_qk = q_offsets[n_q];
    u64 *d_db = nullptr, *d_q = nullptr, found = 0;
    ksp_edge *d_edges = nullptr, *d_sorted = nullptr, *h_edges = nullptr;
    void* tmp = nullptr;
    size_t tb = 0;
    ksp_query_stats S;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // a first guess that a few hits per query satisfy; the call reports the exact size when it does not
    u64 capacity = std::max<u64>(4096, 8ull * ((u64)n_db + n_q));
    if ((rc = ksp::device_fits(who, 8ull * (n_dbk + n_qk + 2) + 16ull * capacity, "the keys of both sides and the first edge buffer"))) return rc;
    if ((rc = A.alloc(&d_db, (size_t)n_dbk + 1)) || (rc = A.alloc(&d_q, (size_t)n_qk + 1)) || (rc = A.alloc(&d_edges, (size_t)capacity))) return rc;
    KSP_TRY_HIP(hipMemcpy(d_db, db_keys, (size_t)n_dbk * 8, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemcpy(d_q, q_keys, (size_t)n_qk * 8, hipMemcpyHostToDevice));
    rc = query_on_device(who, d_db, db_offsets, n_db, d_q, q_offsets, n_q, mode, d_edges, capacity, &found, &S);
    if (rc == KSP_E_OVERFLOW) {   // once more, at the exact size
        KSP_TRY_HIP(A.release(d_edges));
        d_edges = nullptr;
        capacity = found;
        if ((rc = ksp::device_fits(who, 16ull * capacity, "the edges"))) return rc;
        if ((rc = A.alloc(&d_edges, (size_t)capacity))) return rc;
        rc = query_on_device(who, d_db, db_offsets, n_db, d_q, q_offsets, n_q, mode, d_edges, capacity, &found, &S);
    }
    if (rc != KSP_OK) goto done;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    h_edges = (ksp_edge*)std::malloc((size_t)std::max<u64>(found, 1) * sizeof(ksp_edge));
    if (!h_edges) { ksp::set_error(std::string(who) + ": out of host memory"); rc = KSP_E_LIMIT; goto done; }
    if (found) {
        KSP_TRY_HIP(rocprim::merge_sort(nullptr, tb, (const ksp_edge*)d_edges, d_sorted, (size_t)found, EdgeBefore(), (hipStream_t) nullptr));
        tb = std::max<size_t>(tb, 8);
        if ((rc = ksp::device_fits(who, 16ull * found + tb, "the sorted edges and the sort's scratch"))) goto done;
        if ((rc = A.alloc(&d_sorted, (size_t)found)) || (rc = A.alloc_bytes(&tmp, tb))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        KSP_TRY_HIP(rocprim::merge_sort(tmp, tb, (const ksp_edge*)d_edges, d_sorted, (size_t)found, EdgeBefore(), (hipStream_t) nullptr));
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipMemcpy(h_edges, d_sorted, (size_t)found * sizeof(ksp_edge), hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipEventElapsedTime(&S.ms_sort, ev0, ev1));
    }
    *edges = h_edges;
    h_edges = nullptr;
    *n_edges = found;
    if (stats) *stats = S;
done:
    if (h_edges) std::free(h_edges);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}
