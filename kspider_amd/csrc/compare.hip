// Compare: counted sketches against each other.  Query mode's table and probe (query.hip), with counters that carry
// sums of abundances and of their products: for every pair of the mode that shares a hash the row is (shared, dot, mass_1,
// mass_2), and per source the call returns Σ a and Σ a² (include/kspider_amd.h has the definition).  Everything is an integer.
//
//   check    k_compare_check, a workgroup per source of both sides: a run that is not strictly ascending, an abundance of 0 ->
//            the smallest such source, KSP_E_ARG; a run out of order anywhere is reported before an abundance of 0 anywhere.
//   totals   k_compare_totals, a workgroup per source: Σ a (u64) and Σ a² with a carry word.  A carry is Σ a² >= 2^64:
//            KSP_E_LIMIT before any probe.  Without one every dot and mass is below 2^64 and the probe's adds cannot wrap.
//   table    per tile of at most KSP_COMPARE_TILE consecutive queries: query_table.hip.h, as query mode builds it.
//   holders  k_compare_holders: ta[h] = the abundance of the query entry that holder slot h stands for (1 for a flat side).
//            Strict ascent makes the holder of an entry unique, so every slot is written exactly once.
//   probe    k_compare_probe, the shape of k_query_probe: a wave per short source, a workgroup per long one, kProbeKeys look-ups
//            in flight, a touched list, mode 1's min_tag skip.  Per query of the tile: cnt (u32) and dot, m1, m2 (u64, LDS 64-bit
//            adds); the first touch is detected on cnt.  Emission: one ballot, one returning add on a 64-bit cursor per wave.
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

constexpr u32 kTileMax = KSP_COMPARE_TILE_MAX;   // queries per tile: 28 bytes of counters each, 14 KiB per group
constexpr u32 kListMax = KSP_COMPARE_LIST_MAX;   // touched-list entries per group: 1 KiB
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr u32 kGroupBytes = kTileMax * (4 + 3 * 8) + kListMax * 4;
// the wave kernel holds four groups: 4 x (14 + 1) KiB + 16 bytes = 61 456; two of its workgroups fit the 160 KiB of a CU
static_assert(kGroupBytes == 15360, "28 bytes per query of the tile, 4 per list entry");
static_assert(2 * (kWaves * kGroupBytes + 64) <= 160 * 1024, "two workgroups per CU");
static_assert(kWaves * kGroupBytes + 64 <= 64 * 1024, "static LDS of one workgroup");

// both sides of a call as the kernels see them: source s < n_db is the database's, the others are queries
struct CSides {
    const u64 *db_keys, *db_off, *q_keys, *q_off;
    const u32 *db_abund, *q_abund;   // NULL: every abundance is 1
    u32 n_db, n_q;
};

// bad[0] / bad[1] = the smallest source with a run that is not strictly ascending / with an abundance of 0 (start: 0xFFFFFFFF)
__global__ __launch_bounds__(kThreads) void k_compare_check(const CSides S, u32* __restrict__ bad) {
    const u64 n = (u64)S.n_db + S.n_q;
    for (u64 s = blockIdx.x; s < n; s += gridDim.x) {
        const bool is_q = s >= S.n_db;
        const u32 i = is_q ? (u32)(s - S.n_db) : (u32)s;
        const u64* const keys = is_q ? S.q_keys : S.db_keys;
        const u32* const abund = is_q ? S.q_abund : S.db_abund;
        const u64 o0 = is_q ? S.q_off[i] : S.db_off[i], o1 = is_q ? S.q_off[i + 1] : S.db_off[i + 1];
        bool order = false, zero = false;
        for (u64 e = o0 + threadIdx.x; e < o1; e += kThreads) {
            if (e > o0 && keys[e] <= keys[e - 1]) order = true;
            if (abund && abund[e] == 0) zero = true;
        }
        if (order) atomicMin(&bad[0], (u32)s);
        if (zero) atomicMin(&bad[1], (u32)s);
    }
}

// sum[s] = Σ a, sq[s] = the low 64 bits of Σ a², carry[s] = the times that word wrapped: not 0 means Σ a² >= 2^64.  (An add
// wraps at most once, so the u32 holds the carries of any run whose Σ a itself stays below 2^64.)
__global__ __launch_bounds__(kThreads) void k_compare_totals(const CSides S, u64* __restrict__ sum, u64* __restrict__ sq, u32* __restrict__ carry) {
    __shared__ unsigned long long s_sum, s_sq;
    __shared__ u32 s_carry;
    const u64 n = (u64)S.n_db + S.n_q;
    for (u64 s = blockIdx.x; s < n; s += gridDim.x) {
        const bool is_q = s >= S.n_db;
        const u32 i = is_q ? (u32)(s - S.n_db) : (u32)s;
        const u32* const abund = is_q ? S.q_abund : S.db_abund;
        const u64 o0 = is_q ? S.q_off[i] : S.db_off[i], o1 = is_q ? S.q_off[i + 1] : S.db_off[i + 1];
        if (threadIdx.x == 0) { s_sum = 0; s_sq = 0; s_carry = 0; }
        __syncthreads();
        u64 a_sum = 0, a_sq = 0;
        u32 a_carry = 0;
        for (u64 e = o0 + threadIdx.x; e < o1; e += kThreads) {
            const u64 a = abund ? abund[e] : 1;
            a_sum += a;
            a_sq += a * a;   // a² < 2^64
            a_carry += a_sq < a * a;
        }
        if (a_sum) {   // (a lane that read an entry: abundances of 0 were refused, and a sum of 0 adds nothing)
            atomicAdd(&s_sum, (unsigned long long)a_sum);
            const u64 before = atomicAdd(&s_sq, (unsigned long long)a_sq);
            a_carry += before + a_sq < before;
            if (a_carry) atomicAdd(&s_carry, a_carry);
        }
        __syncthreads();
        if (threadIdx.x == 0) { sum[s] = s_sum; sq[s] = s_sq; carry[s] = s_carry; }
        __syncthreads();
    }
}

// ta[h] = the abundance of entry e0 + i of the tile, h = the holder slot of (its key, its query); tag[] is k_query_tag's.  The
// runs ascend strictly, so no two entries share a slot.
__global__ __launch_bounds__(kThreads) void k_compare_holders(const QTable T, const u64* __restrict__ q_keys, const u32* __restrict__ q_abund, const u32* __restrict__ tag,
                                                              const u64 e0, const u32 E, const u32 H, u32* __restrict__ ta) {
    const u64 span = (u64)gridDim.x * kThreads;
    for (u64 i0 = (u64)blockIdx.x * kThreads + threadIdx.x; i0 < E; i0 += span * kProbeKeys) {
        u64 k[kProbeKeys];
        bool live[kProbeKeys];
        u32 at[kProbeKeys];
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            const u64 i = i0 + (u64)x * span;
            live[x] = i < E;
            k[x] = live[x] ? q_keys[e0 + i] : 0;
        }
        query_lookup(T, k, live, at);
#pragma unroll
        for (int x = 0; x < kProbeKeys; ++x) {
            if (!live[x]) continue;   // (never for an entry of the tile: the table holds its key)
            const u64 i = i0 + (u64)x * span;
            const u32 mine = tag[i];
            u32 lo = T.toff[at[x]], hi = T.toff[at[x] + 1];   // the holders of a key ascend
            while (lo < hi) {
                const u32 mid = lo + (hi - lo) / 2;
                if (T.tq[mid] < mine) lo = mid + 1; else hi = mid;
            }
            if (lo < H && lo < T.toff[at[x] + 1] && T.tq[lo] == mine) ta[lo] = q_abund ? q_abund[e0 + i] : 1u;
        }
    }
}

// what a probe kernel reads and writes besides the table
struct CProbe {
    CSides S;
    const u32* ta;     // per holder slot of the tile's table: its abundance
    const u32* list;   // the probe sources of this kernel, in the common numbering
    u32 n_list;
    u32 list_cap;      // touched-list capacity, 1 .. kListMax
    ksp_wedge* rows;
    u64 capacity;
    unsigned long long* cursor;      // rows appended so far, the ones that found no room included
    unsigned long long* overflows;   // sources whose touched list overflowed
};

// One group per probe source: a wave (kWave, four groups per workgroup) or the whole workgroup.  For query t of the tile cnt[t] =
// the keys the source shares with it, dot[t] / m1[t] / m2[t] = Σ over them of a_source · a_query / a_source / a_query;
// list[0 .. min(*n, cap)): the queries whose cnt left 0.
template <bool kWave>
__global__ __launch_bounds__(kThreads) void k_compare_probe(const QTable T, const CProbe P) {
    constexpr u32 kGroups = kWave ? kWaves : 1;
    constexpr u32 kLanes = kWave ? 64 : kThreads;
    __shared__ unsigned long long s_dot[kGroups][kTileMax], s_m1[kGroups][kTileMax], s_m2[kGroups][kTileMax];
    __shared__ u32 s_cnt[kGroups][kTileMax];
    __shared__ u32 s_list[kGroups][kListMax];
    __shared__ u32 s_n[kGroups];
    const u32 g = kWave ? threadIdx.x >> 6 : 0, t = kWave ? threadIdx.x & 63 : threadIdx.x, lane = threadIdx.x & 63;
    unsigned long long* const dot = s_dot[g];
    unsigned long long* const m1 = s_m1[g];
    unsigned long long* const m2 = s_m2[g];
    u32* const cnt = s_cnt[g];
    u32* const list = s_list[g];
    u32* const n = &s_n[g];
    for (u32 j = t; j < T.nq; j += kLanes) { cnt[j] = 0; dot[j] = 0; m1[j] = 0; m2[j] = 0; }
    if (t == 0) *n = 0;
    query_group_sync<kWave>();
    const CSides& S = P.S;
    const u64 first = kWave ? (u64)blockIdx.x * kWaves + g : blockIdx.x, stride = kWave ? (u64)gridDim.x * kWaves : gridDim.x;
    for (u64 i = first; i < P.n_list; i += stride) {
        const u32 p = P.list[i];
        const bool is_q = p >= S.n_db;
        const u32 qi = is_q ? p - S.n_db : 0;
        if (is_q && (u64)qi + 1 >= (u64)T.q0 + T.nq) continue;   // (the same for the whole group) no holder of this tile is above query qi
        const u32 min_tag = is_q && qi >= T.q0 ? qi - T.q0 + 1 : 0;   // mode 1: a probing query skips the holders j <= i
        const u64* const keys = is_q ? S.q_keys : S.db_keys;
        const u32* const abund = is_q ? S.q_abund : S.db_abund;
        const u64 o0 = is_q ? S.q_off[qi] : S.db_off[p], o1 = is_q ? S.q_off[qi + 1] : S.db_off[p + 1];
        for (u64 e = o0 + t; e < o1; e += (u64)kLanes * kProbeKeys) {
            u64 k[kProbeKeys], a[kProbeKeys];
            bool live[kProbeKeys];
            u32 at[kProbeKeys];
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x) {
                const u64 ex = e + (u64)x * kLanes;
                live[x] = ex < o1;
                k[x] = live[x] ? keys[ex] : 0;
                a[x] = live[x] && abund ? abund[ex] : 1;
            }
            query_lookup(T, k, live, at);
#pragma unroll
            for (int x = 0; x < kProbeKeys; ++x) {
                if (!live[x]) continue;
                const u32 h1 = T.toff[at[x] + 1];
                for (u32 h = T.toff[at[x]]; h < h1; ++h) {
                    const u32 tag = T.tq[h];
                    if (tag < min_tag || tag >= T.nq) continue;   // (a tag is below nq by construction)
                    const u64 b = P.ta[h];
                    atomicAdd(&dot[tag], (unsigned long long)(a[x] * b));
                    atomicAdd(&m1[tag], (unsigned long long)a[x]);
                    atomicAdd(&m2[tag], (unsigned long long)b);
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
            u64 d = 0, w1 = 0, w2 = 0;
            if (j < count) {
                tag = over ? j : list[j];
                c = cnt[tag];
                if (c) {
                    d = dot[tag]; w1 = m1[tag]; w2 = m2[tag];
                    cnt[tag] = 0; dot[tag] = 0; m1[tag] = 0; m2[tag] = 0;
                }
            }
            const unsigned long long have = __ballot(c != 0);
            if (!have) continue;   // (the whole wave)
            unsigned long long at = 0;
            if (lane == (u32)__ffsll((long long)have) - 1) at = atomicAdd(P.cursor, (unsigned long long)__popcll(have));
            const int src = __ffsll((long long)have) - 1;
            const u32 at_lo = (u32)__shfl((int)(u32)at, src), at_hi = (u32)__shfl((int)(u32)(at >> 32), src);
            const u64 slot = (((u64)at_hi << 32) | at_lo) + (u64)__popcll(have & ((1ull << lane) - 1));
            if (c && slot < P.capacity) P.rows[slot] = ksp_wedge{p, S.n_db + T.q0 + tag, (u64)c, d, w1, w2};
        }
        query_group_sync<kWave>();
    }
}

struct WedgeBefore {
    __host__ __device__ bool operator()(const ksp_wedge& a, const ksp_wedge& b) const {
        return a.source_1 != b.source_1 ? a.source_1 < b.source_1 : a.source_2 < b.source_2;
    }
};

const u64 kNoOffsets[1] = {0};   // the offsets of a database without a source

// what both entry points refuse before a device is chosen; *db_off becomes kNoOffsets for n_db = 0
int check_compare_args(const char* who, const void* db_keys, const u64** db_off, const u32 n_db, const void* q_keys, const u64* q_off, const u32 n_q, const int mode,
                       const void* n_rows) {
    if (!q_keys || !q_off || !n_rows || (n_db && (!db_keys || !*db_off))) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_q == 0) { ksp::set_error(std::string(who) + ": no query"); return KSP_E_ARG; }
    if (mode != KSP_QUERY_CROSS && mode != KSP_QUERY_CROSS_AND_SELF) {
        ksp::set_error(std::string(who) + ": mode is KSP_QUERY_CROSS (0) or KSP_QUERY_CROSS_AND_SELF (1)");
        return KSP_E_ARG;
    }
    if (n_db == 0 && mode == KSP_QUERY_CROSS) { ksp::set_error(std::string(who) + ": no database source (only KSP_QUERY_CROSS_AND_SELF compares the queries with each other)"); return KSP_E_ARG; }
    if ((u64)n_db + n_q > 0xFFFFFFFEull) { ksp::set_error(std::string(who) + ": more than 2^32 - 2 sources"); return KSP_E_LIMIT; }   // (from the counts alone)
    if (n_db == 0) *db_off = kNoOffsets;
    if (const int rc = check_offsets(who, "database", *db_off, n_db)) return rc;
    return check_offsets(who, "query", q_off, n_q);
}

// "query source 3" / "database source 0" of source s in the common numbering
std::string source_name(const u32 s, const u32 n_db) { return s < n_db ? "database source " + std::to_string(s) : "query source " + std::to_string(s - n_db); }

// The comparison on the CURRENT device; the arguments have passed check_compare_args.  S: keys and abundances on the device, the
// offsets still the host's.
int compare_on_device(const char* who, const CSides& S, const int mode, ksp_wedge* d_rows, const u64 capacity, u64* n_rows, u64* h_sum, u64* h_sumsq,
                      ksp_compare_stats* stats) {
    int rc = KSP_OK;
    const u32 n_db = S.n_db, n_q = S.n_q;
    const u64 *const h_db_off = S.db_off, *const h_q_off = S.q_off;
    const u64 n_src = (u64)n_db + n_q;
    ksp_compare_stats C;
    std::memset(&C, 0, sizeof C);
    u64 tile = 0, long_run = 0, list_cap = 0;
    ksp::WorkgroupCap G;
    if ((rc = env_number(who, "KSP_COMPARE_TILE", kTileMax, 1, kTileMax, &tile)) || (rc = env_number(who, "KSP_COMPARE_LONG_RUN", KSP_QUERY_LONG_RUN, 1, ~0ull, &long_run)) ||
        (rc = env_number(who, "KSP_COMPARE_LIST", kListMax, 1, kListMax, &list_cap)))
        return rc;
    u32 n_tiles = 0;
    u64 e_max = 0;
    if ((rc = query_tiles(who, h_q_off, n_q, tile, &n_tiles, &e_max))) {
        if (rc == KSP_E_LIMIT) ksp::set_error(std::string(who) + ": a query tile of 2^31 entries or more (lower KSP_COMPARE_TILE)");
        return rc;
    }
    if ((rc = ksp::workgroup_cap("KSP_COMPARE_MAX_WORKGROUPS", who, G))) return rc;
    // the probe sources by run length: the database's, then in mode 1 the queries (the last query has no query above it)
    std::vector<u32> probes[2];   // [0] short, [1] long
    query_split_sources(h_db_off, n_db, long_run, 0, probes);
    if (mode == KSP_QUERY_CROSS_AND_SELF) query_split_sources(h_q_off, n_q - 1, long_run, n_db, probes);
    C.n_db = n_db; C.n_q = n_q; C.db_entries = h_db_off[n_db]; C.q_entries = h_q_off[n_q];
    C.short_sources = probes[0].size(); C.long_sources = probes[1].size();
    C.tile = (u32)tile; C.long_run = long_run; C.list_capacity = (u32)list_cap;

    ksp::DeviceArena A;
    ksp::Events<4> ev;
    QTableBufs B;
    B.e_max = e_max;
    if ((rc = query_table_scratch(e_max, &B.tb))) return rc;
    B.tb = std::max<size_t>(B.tb, 8);
    // ---- everything the call holds, sized and checked first: query mode's list (8 per source, 4 per probe source, 40 per entry of
    // the largest tile, the directory, the scratch), 4 more per entry of the largest tile (ta), 24 per source (the totals)
    if ((rc = ksp::device_fits(who, (8ull + 24ull) * (n_src + 2) + 4ull * (probes[0].size() + probes[1].size()) + B.bytes() + 4ull * (e_max + 1) + B.tb + 64,
                               "32 per source, 4 per probe source, 44 per entry of the largest query tile, its directory, the sort's scratch")))
        return rc;
    u64 *d_db_off = nullptr, *d_q_off = nullptr, *d_sum = nullptr, *d_sq = nullptr;
    u32 *d_list[2] = {nullptr, nullptr}, *d_carry = nullptr, *d_bad = nullptr, *d_ta = nullptr;
    unsigned long long* d_count = nullptr;   // [0] the cursor, [1] the list overflows
    if ((rc = query_upload_front(A, h_db_off, n_db, h_q_off, n_q, probes, &d_db_off, &d_q_off, d_list)) || (rc = A.alloc(&d_count, 2)) || (rc = A.alloc(&d_sum, (size_t)n_src)) ||
        (rc = A.alloc(&d_sq, (size_t)n_src)) || (rc = A.alloc(&d_carry, (size_t)n_src)) || (rc = A.alloc(&d_bad, 2)) || (rc = A.alloc(&d_ta, (size_t)e_max + 1)))
        return rc;
    if (e_max && ((rc = query_table_alloc(A, B)) || (rc = A.alloc_bytes(&B.tmp, B.tb)))) return rc;
    KSP_HIP(hipMemset(d_count, 0, 16));
    KSP_HIP(hipMemset(d_bad, 0xFF, 8));
    if ((rc = ev.create())) return rc;
    CSides D = S;   // what the kernels get: the offsets on the device too
    D.db_off = d_db_off; D.q_off = d_q_off;

    // ---- the check and the totals: before any probe
    std::vector<u64> sum((size_t)n_src), sq((size_t)n_src);
    {
        std::vector<u32> carry((size_t)n_src);
        u32 bad[2] = {0, 0};
        const unsigned grid = G.grid_of(n_src);
        float ms = 0;
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        hipLaunchKernelGGL(k_compare_check, dim3(grid), dim3(kThreads), 0, nullptr, D, d_bad);
        hipLaunchKernelGGL(k_compare_totals, dim3(grid), dim3(kThreads), 0, nullptr, D, d_sum, d_sq, d_carry);
        KSP_HIP(hipGetLastError());
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        KSP_HIP(hipMemcpy(bad, d_bad, 8, hipMemcpyDeviceToHost));
        KSP_HIP(hipMemcpy(sum.data(), d_sum, (size_t)n_src * 8, hipMemcpyDeviceToHost));
        KSP_HIP(hipMemcpy(sq.data(), d_sq, (size_t)n_src * 8, hipMemcpyDeviceToHost));
        KSP_HIP(hipMemcpy(carry.data(), d_carry, (size_t)n_src * 4, hipMemcpyDeviceToHost));
        KSP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        C.ms_totals = ms;
        if (bad[0] != 0xFFFFFFFFu) { ksp::set_error(std::string(who) + ": the run of " + source_name(bad[0], n_db) + " is not strictly ascending"); return KSP_E_ARG; }
        if (bad[1] != 0xFFFFFFFFu) { ksp::set_error(std::string(who) + ": " + source_name(bad[1], n_db) + " has an abundance of 0"); return KSP_E_ARG; }
        for (u64 s = 0; s < n_src; ++s)
            if (carry[(size_t)s]) {
                ksp::set_error(std::string(who) + ": the squared abundances of " + source_name((u32)s, n_db) + " sum to 2^64 or more");
                return KSP_E_LIMIT;
            }
    }
    if (h_sum) std::memcpy(h_sum, sum.data(), (size_t)n_src * 8);
    if (h_sumsq) std::memcpy(h_sumsq, sq.data(), (size_t)n_src * 8);

    for (u32 t = 0; t < n_tiles; ++t) {
        const u32 q0 = (u32)((u64)t * tile), nq = (u32)(std::min<u64>((u64)q0 + tile, n_q) - q0);
        const u64 e0 = h_q_off[q0];
        const u32 E = (u32)(h_q_off[q0 + nq] - e0);
        if (E == 0) continue;   // a tile of empty queries shares nothing
        // ---- the table
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        QTable T;
        u32 U = 0, H = 0;
        if ((rc = query_table_build(who, G, B, S.q_keys, d_q_off, q0, nq, e0, E, &T, &U, &H))) return rc;
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        // ---- the abundance of every (hash, query) of the tile at its holder slot
        hipLaunchKernelGGL(k_compare_holders, dim3(G.grid_of(((u64)E + kThreads * kProbeKeys - 1) / (kThreads * kProbeKeys))), dim3(kThreads), 0, nullptr, T, S.q_keys, S.q_abund,
                           (const u32*)B.tag, e0, E, H, d_ta);
        KSP_HIP(hipGetLastError());
        KSP_HIP(hipEventRecord(ev[2], nullptr));
        // ---- the probe: every probe source against this tile
        CProbe P{D, d_ta, nullptr, 0, (u32)list_cap, d_rows, d_rows ? capacity : 0, &d_count[0], &d_count[1]};
        if (!probes[0].empty()) {
            P.list = d_list[0]; P.n_list = (u32)probes[0].size();
            hipLaunchKernelGGL(k_compare_probe<true>, dim3(G.grid_of(((u64)P.n_list + kWaves - 1) / kWaves)), dim3(kThreads), 0, nullptr, T, P);
        }
        if (!probes[1].empty()) {
            P.list = d_list[1]; P.n_list = (u32)probes[1].size();
            hipLaunchKernelGGL(k_compare_probe<false>, dim3(G.grid_of(P.n_list)), dim3(kThreads), 0, nullptr, T, P);
        }
        KSP_HIP(hipGetLastError());
        KSP_HIP(hipEventRecord(ev[3], nullptr));
        KSP_HIP(hipEventSynchronize(ev[3]));
        float ms_t = 0, ms_h = 0, ms_p = 0;
        KSP_HIP(hipEventElapsedTime(&ms_t, ev[0], ev[1]));
        KSP_HIP(hipEventElapsedTime(&ms_h, ev[1], ev[2]));
        KSP_HIP(hipEventElapsedTime(&ms_p, ev[2], ev[3]));
        C.ms_table += ms_t; C.ms_holders += ms_h; C.ms_probe += ms_p;
        C.table_keys += U; C.table_holders += H; ++C.passes;
    }
    unsigned long long h_count[2] = {0, 0};
    KSP_HIP(hipMemcpy(h_count, d_count, 16, hipMemcpyDeviceToHost));
    C.edges = h_count[0]; C.list_overflows = h_count[1];
    *n_rows = h_count[0];
    if (stats) *stats = C;
    if (h_count[0] > capacity) {
        ksp::set_error(std::string(who) + ": " + std::to_string(h_count[0]) + " rows, room for " + std::to_string(capacity));
        return KSP_E_OVERFLOW;
    }
    return KSP_OK;
}

// host array `src` of n values as *dst in the arena (an entry more: never an allocation of 0 bytes); a NULL src stays NULL
template <class V>
int upload(ksp::DeviceArena& A, const V* src, const u64 n, const V** dst) {
    V* p = nullptr;
    *dst = nullptr;
    if (!src) return KSP_OK;
    if (const int rc = A.alloc(&p, (size_t)n + 1)) return rc;
    KSP_HIP(hipMemcpy(p, src, (size_t)n * sizeof(V), hipMemcpyHostToDevice));
    *dst = p;
    return KSP_OK;
}

}  // namespace

extern "C" int ksp_compare_device(int device, const uint64_t* d_db_keys, const uint32_t* d_db_abund, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys,
                                  const uint32_t* d_q_abund, const uint64_t* h_q_offsets, uint32_t n_q, int mode, ksp_wedge* d_rows, uint64_t capacity, uint64_t* n_rows,
                                  uint64_t* h_sum, uint64_t* h_sumsq, ksp_compare_stats* stats) {
    const char* who = "ksp_compare_device";
    if (const int rc = check_compare_args(who, d_db_keys, &h_db_offsets, n_db, d_q_keys, h_q_offsets, n_q, mode, n_rows)) return rc;
    if (!d_rows && capacity) { ksp::set_error(std::string(who) + ": d_rows is NULL but capacity is not 0"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    const CSides S{d_db_keys, h_db_offsets, d_q_keys, h_q_offsets, n_db ? d_db_abund : nullptr, d_q_abund, n_db, n_q};
    return compare_on_device(who, S, mode, d_rows, capacity, n_rows, h_sum, h_sumsq, stats);
}

extern "C" int ksp_compare_host(const uint64_t* db_keys, const uint32_t* db_abund, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint32_t* q_abund,
                                const uint64_t* q_offsets, uint32_t n_q, int mode, int device, ksp_wedge** rows, uint64_t* n_rows, uint64_t* sum, uint64_t* sumsq,
                                ksp_compare_stats* stats) {
    const char* who = "ksp_compare_host";
    if (!rows) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (const int rc = check_compare_args(who, db_keys, &db_offsets, n_db, q_keys, q_offsets, n_q, mode, n_rows)) return rc;
    u64 capacity = 0;   // a first guess that a few hits per source satisfy; the call reports the exact size when it does not
    if (const int rc = env_number(who, "KSP_COMPARE_FIRST_CAPACITY", std::max<u64>(4096, 8ull * ((u64)n_db + n_q)), 1, 1ull << 40, &capacity)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::Events<2> ev;
    const u64 n_dbk = db_offsets[n_db], n_qk = q_offsets[n_q];
    u64 found = 0;
    ksp_wedge* d_rows = nullptr;
    ksp_compare_stats C;
    CSides S{nullptr, db_offsets, nullptr, q_offsets, nullptr, nullptr, n_db, n_q};
    if ((rc = ksp::device_fits(who, 12ull * (n_dbk + n_qk + 4) + sizeof(ksp_wedge) * capacity, "the keys and abundances of both sides and the first row buffer"))) return rc;
    // (a database without a source has no keys: its pointers stay NULL and are never read)
    if ((rc = upload(A, n_db ? db_keys : nullptr, n_dbk, &S.db_keys)) || (rc = upload(A, q_keys, n_qk, &S.q_keys)) ||
        (rc = upload(A, n_db ? db_abund : nullptr, n_dbk, &S.db_abund)) || (rc = upload(A, q_abund, n_qk, &S.q_abund)) || (rc = A.alloc(&d_rows, (size_t)capacity)))
        return rc;
    rc = compare_on_device(who, S, mode, d_rows, capacity, &found, sum, sumsq, &C);
    if (rc == KSP_E_OVERFLOW) {   // once more, at the exact size
        KSP_HIP(A.release(d_rows));
        d_rows = nullptr;
        capacity = found;
        if ((rc = ksp::device_fits(who, sizeof(ksp_wedge) * capacity, "the rows"))) return rc;
        if ((rc = A.alloc(&d_rows, (size_t)capacity))) return rc;
        rc = compare_on_device(who, S, mode, d_rows, capacity, &found, sum, sumsq, &C);
    }
    if (rc != KSP_OK) return rc;
    if ((rc = ev.create())) return rc;
    std::unique_ptr<ksp_wedge, decltype(&std::free)> h_rows((ksp_wedge*)std::malloc((size_t)std::max<u64>(found, 1) * sizeof(ksp_wedge)), &std::free);
    if (!h_rows) { ksp::set_error(std::string(who) + ": out of host memory"); return KSP_E_LIMIT; }
    if (found) {
        ksp_wedge* d_sorted = nullptr;
        void* tmp = nullptr;
        size_t tb = 0;
        KSP_HIP(rocprim::merge_sort(nullptr, tb, (const ksp_wedge*)d_rows, d_sorted, (size_t)found, WedgeBefore(), (hipStream_t) nullptr));
        tb = std::max<size_t>(tb, 8);
        if ((rc = ksp::device_fits(who, sizeof(ksp_wedge) * found + tb, "the sorted rows and the sort's scratch"))) return rc;
        if ((rc = A.alloc(&d_sorted, (size_t)found)) || (rc = A.alloc_bytes(&tmp, tb))) return rc;
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        KSP_HIP(rocprim::merge_sort(tmp, tb, (const ksp_wedge*)d_rows, d_sorted, (size_t)found, WedgeBefore(), (hipStream_t) nullptr));
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        KSP_HIP(hipMemcpy(h_rows.get(), d_sorted, (size_t)found * sizeof(ksp_wedge), hipMemcpyDeviceToHost));
        KSP_HIP(hipEventElapsedTime(&C.ms_sort, ev[0], ev[1]));
    }
    *rows = h_rows.release();
    *n_rows = found;
    if (stats) *stats = C;
    return KSP_OK;
}
