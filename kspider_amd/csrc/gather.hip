// Gather: the greedy minimum-set-cover of every query by database sources — take the source that covers most of
// what is left of the query, remove its hashes, ask again — on the database that stays in HBM.  Exact integers, a total tie
// rule (the smaller source), so one well-defined table whatever the scheduling.
//
// Per tile of queries (the tiling and the table are query mode's: query_table.hip.h):
//   candidates  one sweep of the database against the tile's table counts, per source, the hashes it shares with every query
//               (u32 counters in LDS, a wave per short source, a workgroup per long one).  A (source, query) pair whose overlap
//               reaches min_hashes is a candidate: (query << 32 | source, overlap) appended through one returning add per
//               wave; the others can never win and are only counted.  Sorted by that word, a candidate's index orders the
//               sources within its query; an exclusive scan of the overlaps gives every candidate a segment.
//   segments    a second sweep, over the sources that have a candidate only, counts again and then turns the counter of a
//               touched query into the cursor of its segment (the candidate is found by binary search in the sorted words; a
//               pair below min_hashes gets kNone).  A second walk over the source's hashes writes, for every hit, the holder
//               slot h (the index into the table's tq[], unique per (key, query) membership) at the cursor's returning add.
//               No second LDS array: the counters ARE the segment bases, and the LDS budget stays query mode's.
//   alive       one bit per holder slot, all set.  Slots of different queries share words: clearing is an atomic AND.
//   a round     for all queries of the tile at once.  count: a wave per live candidate with a short segment, a workgroup per
//               long one, counts the alive slots u of its segment by ballots; u < min_hashes: dead for good (counts only fall);
//               otherwise it offers (u << 32) | ~index to a 64-bit atomicMax per query.  take: a wave per query; the winner's
//               slots are cleared, the row appended, remaining lowered, the offer reset; a query without an offer, or at
//               max_matches, is finished.
//   batches     KSP_GATHER_BATCH rounds are launched back to back; the kernels return at once when the device's counter of live
//               queries is 0; the host reads that counter once per batch, after the live lists were compacted.
//   tail        at KSP_GATHER_TAIL_CANDS live candidates or fewer ONE workgroup of 1 024 threads runs the remaining rounds with
//               __syncthreads() between count and take (k_derep_tail's pattern); KSP_GATHER_TAIL=0: batches to the end.
//   weighted    (ksp_gather_abund_*) the queries carry an abundance per hash.  k_gather_habund puts it at the holder slot
//               of its (hash, query); the take (gather_take<true>: k_gather_take_w, k_gather_tail_w) sums a and a^2 over the slots
//               it clears, compacts their abundances into the winner's own segment and selects the median there.  The greedy, the
//               counts and every kernel of the unweighted call are what they were.
// Every loop is bounded by a size the host computed; no workgroup waits on another; stores are plain vector stores.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"
#include "query_table.hip.h"

namespace {

constexpr u32 kTileMax = KSP_QUERY_TILE_MAX;
constexpr u32 kListMax = KSP_QUERY_LIST_MAX;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTailThreads = 1024;
constexpr u32 kTailWaves = kTailThreads / 64;
constexpr u32 kNone = 0xFFFFFFFFu;
// the sweeps hold what query mode's probe holds: 4 x (8 + 2) KiB and a few words per workgroup
static_assert(2 * (kWaves * (kTileMax + kListMax) * 4 + 64) <= 160 * 1024, "two workgroups per CU");
static_assert(kWaves * (kTileMax + kListMax) * 4 + 64 <= 64 * 1024, "static LDS of one workgroup");

// the device's words of a tile (unsigned long long each)
enum : int { kLiveQ = 0, kRounds, kRows, kGo, kFell, kKept0, kKept1, kCands, kDropped, kFill0, kFill1, kCtrlWords };

__device__ inline u32 load_u32(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline unsigned long long load_u64(const unsigned long long* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---------------------------------------------------------------------------------------------------------------- the sweeps
struct GSweep {
    const u64 *db_keys, *db_off;
    const u32* list;   // the sources of this kernel
    u32 n_list;
    u32 list_cap;      // touched-list capacity, 1 .. kListMax
    u32 min_hashes;
    unsigned long long* ctrl;
    // the counting sweep: candidates out
    u64* cand_key;     // (query inside the tile << 32) | source
    u32* cand_ovl;
    u64 cand_cap;
    u32* fill_list;    // the sources of this kernel that have a candidate; its counter: ctrl[fill_word]
    int fill_word;
    // the filling sweep: the sorted candidates in, holder slots out
    const u64* ckey;
    const u64* cbase;  // n_cand + 1
    u32 n_cand;
    u32* seg;
    u32 n_slots;
};

// cnt[t] += the keys of the run [o0, o1) that query t of the tile holds; a query whose counter left 0 goes to the touched list
template <bool kWave>
__device__ inline void gather_count_run(const QTable& T, const u64* __restrict__ keys, const u64 o0, const u64 o1, u32* cnt, u32* list, u32* n, const u32 list_cap,
                                        const u32 t) {
    constexpr u32 kLanes = kWave ? 64 : kThreads;
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
                if (tag >= T.nq) continue;   // (a tag is below nq by construction)
                if (atomicAdd(&cnt[tag], 1u) == 0) {
                    const u32 pos = atomicAdd(n, 1u);
                    if (pos < list_cap) list[pos] = tag;
                }
            }
        }
    }
}

// the index of `word` in the ascending ckey[0 .. n), or kNone
__device__ inline u32 gather_find(const u64* __restrict__ ckey, const u32 n, const u64 word) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + (hi - lo) / 2;
        if (ckey[mid] < word) lo = mid + 1; else hi = mid;
    }
    return lo < n && ckey[lo] == word ? lo : kNone;
}

// One group per source: a wave (kWave, four groups per workgroup) or the whole workgroup.  kFill false: the candidates of the
// source; kFill true: the holder slots of its candidates into their segments.
template <bool kWave, bool kFill>
__global__ __launch_bounds__(kThreads) void k_gather_sweep(const QTable T, const GSweep P) {
    constexpr u32 kGroups = kWave ? kWaves : 1;
    constexpr u32 kLanes = kWave ? 64 : kThreads;
    __shared__ u32 s_cnt[kGroups][kTileMax];
    __shared__ u32 s_list[kGroups][kListMax];
    __shared__ u32 s_n[kGroups];
    __shared__ u32 s_any[kGroups];
    const u32 g = kWave ? threadIdx.x >> 6 : 0, t = kWave ? threadIdx.x & 63 : threadIdx.x, lane = threadIdx.x & 63;
    u32* const cnt = s_cnt[g];
    u32* const list = s_list[g];
    u32* const n = &s_n[g];
    for (u32 j = t; j < T.nq; j += kLanes) cnt[j] = 0;
    if (t == 0) { *n = 0; s_any[g] = 0; }
    query_group_sync<kWave>();
    const u64 first = kWave ? (u64)blockIdx.x * kWaves + g : blockIdx.x, stride = kWave ? (u64)gridDim.x * kWaves : gridDim.x;
    for (u64 i = first; i < P.n_list; i += stride) {
        const u32 p = P.list[i];
        const u64 o0 = P.db_off[p], o1 = P.db_off[p + 1];
        gather_count_run<kWave>(T, P.db_keys, o0, o1, cnt, list, n, P.list_cap, t);
        query_group_sync<kWave>();
        const u32 touched = *n;
        query_group_sync<kWave>();
        if (t == 0) *n = 0;
        const bool over = touched > P.list_cap;   // the list lost entries: one scan over all counters replaces it
        const u32 count = over ? T.nq : touched;
        if (!kFill) {
            for (u32 base = 0; base < count; base += kLanes) {   // (the same trips for every lane of the group)
                const u32 j = base + t;
                u32 tag = 0, c = 0;
                if (j < count) {
                    tag = over ? j : list[j];
                    c = cnt[tag];
                    if (c) cnt[tag] = 0;
                }
                const bool cand = c >= P.min_hashes;   // (min_hashes >= 1: never for c = 0)
                const unsigned long long have = __ballot(cand), low = __ballot(c != 0 && !cand);
                if (low && lane == (u32)__ffsll((long long)low) - 1) atomicAdd(&P.ctrl[kDropped], (unsigned long long)__popcll(low));
                if (!have) continue;   // (the whole wave)
                unsigned long long at = 0;
                const int src = __ffsll((long long)have) - 1;
                if (lane == (u32)src) { at = atomicAdd(&P.ctrl[kCands], (unsigned long long)__popcll(have)); s_any[g] = 1; }
                const u32 at_lo = (u32)__shfl((int)(u32)at, src), at_hi = (u32)__shfl((int)(u32)(at >> 32), src);
                const u64 slot = (((u64)at_hi << 32) | at_lo) + (u64)__popcll(have & ((1ull << lane) - 1));
                if (cand && slot < P.cand_cap) {
                    P.cand_key[slot] = ((u64)tag << 32) | p;
                    P.cand_ovl[slot] = c;
                }
            }
            query_group_sync<kWave>();
            if (t == 0 && s_any[g]) {   // (at most once per source: the list has room for every source of the kernel)
                s_any[g] = 0;
                const unsigned long long pos = atomicAdd(&P.ctrl[P.fill_word], 1ull);
                if (pos < P.n_list) P.fill_list[pos] = p;
            }
            query_group_sync<kWave>();
        } else {
            // the counter of a touched query becomes the cursor of its candidate's segment
            for (u32 j = t; j < count; j += kLanes) {
                const u32 tag = over ? j : list[j];
                const u32 c = cnt[tag];
                if (!c) continue;
                u32 cursor = kNone;
                if (c >= P.min_hashes) {
                    const u32 idx = gather_find(P.ckey, P.n_cand, ((u64)tag << 32) | p);
                    if (idx != kNone) cursor = (u32)P.cbase[idx];
                }
                cnt[tag] = cursor;
            }
            query_group_sync<kWave>();
            for (u64 e = o0 + t; e < o1; e += (u64)kLanes * kProbeKeys) {
                u64 k[kProbeKeys];
                bool live[kProbeKeys];
                u32 at[kProbeKeys];
#pragma unroll
                for (int x = 0; x < kProbeKeys; ++x) {
                    const u64 ex = e + (u64)x * kLanes;
                    live[x] = ex < o1;
                    k[x] = live[x] ? P.db_keys[ex] : 0;
                }
                query_lookup(T, k, live, at);
#pragma unroll
                for (int x = 0; x < kProbeKeys; ++x) {
                    if (!live[x]) continue;
                    const u32 h1 = T.toff[at[x] + 1];
                    for (u32 h = T.toff[at[x]]; h < h1; ++h) {
                        const u32 tag = T.tq[h];
                        if (tag >= T.nq) continue;
                        if (__hip_atomic_load(&cnt[tag], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == kNone) continue;   // (kNone is never a cursor: n_slots < 2^32 - 1)
                        const u32 pos = atomicAdd(&cnt[tag], 1u);
                        if (pos < P.n_slots) P.seg[pos] = h;
                    }
                }
            }
            query_group_sync<kWave>();
            for (u32 j = t; j < count; j += kLanes) cnt[over ? j : list[j]] = 0;
            query_group_sync<kWave>();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the rounds
struct GRound {
    const u64* ckey;    // n_cand sorted candidates: (query inside the tile << 32) | source
    const u32* covl;    // their overlaps = segment lengths
    const u64* cbase;   // their segments' first slots in seg[]
    const u32* seg;     // holder slots
    u32* alive;         // one bit per holder slot
    u32* cdead;         // per candidate: taken, or fallen below min_hashes
    unsigned long long* best;   // per query of the tile: the best offer of the round, 0: none
    u32 *qrank, *qrem, *qdone;  // per query: rows so far, |R|, finished
    u32 n_cand, nq, q0, min_hashes, max_matches;
    ksp_gather_row* rows;       // the tile's rows in the order they were found
    u32 rows_cap;
    unsigned long long* ctrl;
};

// the alive slots of candidate c's segment among the entries first + lane, first + lane + stride, ...: the same for the whole wave
__device__ inline u32 gather_alive(const GRound& R, const u32 c, const u32 first, const u32 stride, const u32 lane) {
    const u64 base = R.cbase[c];
    const u32 len = R.covl[c];
    u32 u = 0;
    for (u32 i0 = first; i0 < len; i0 += stride) {   // (the same trips for every lane of the wave)
        const u32 i = i0 + lane;
        bool bit = false;
        if (i < len) {
            const u32 h = R.seg[base + i];
            bit = (load_u32(&R.alive[h >> 5]) >> (h & 31)) & 1u;
        }
        u += (u32)__popcll(__ballot(bit));
    }
    return u;
}

// is candidate c still in the running?  (the same answer for every lane that asks in one round)
__device__ inline bool gather_is_live(const GRound& R, const u32 c) {
    return c < R.n_cand && !load_u32(&R.cdead[c]) && !load_u32(&R.qdone[(u32)(R.ckey[c] >> 32)]);
}

// what ONE lane does with the count u of candidate c
__device__ inline void gather_offer(const GRound& R, const u32 c, const u32 u) {
    if (u < R.min_hashes) {
        R.cdead[c] = 1;
        atomicAdd(&R.ctrl[kFell], 1ull);
    } else {
        atomicMax(&R.best[(u32)(R.ckey[c] >> 32)], ((unsigned long long)u << 32) | (u32)~c);
    }
}

// ---- the weighted take: what a round's row says about the abundances of the hashes it takes
struct GAbund {
    const u32* habund;            // per holder slot: the abundance of its hash in its query
    u32* vals;                    // = seg: the words of a taken segment are dead and hold the abundances it took
    unsigned long long* qwfound;  // per query of the tile: w_found so far
    ksp_gather_wrow* rows;        // the tile's rows in the order they were found
};

__device__ inline u64 shfl_down_u64(const u64 v, const int d) {
    return ((u64)(u32)__shfl_down((int)(u32)(v >> 32), d) << 32) | (u32)__shfl_down((int)(u32)v, d);
}

// habund[h] = the abundance of entry e0 + i of the tile, h = the holder slot of (its key, its query).  tag[] is k_query_tag's.
__global__ __launch_bounds__(kThreads) void k_gather_habund(const QTable T, const u64* __restrict__ q_keys, const u32* __restrict__ q_abund, const u32* __restrict__ tag,
                                                            const u64 e0, const u32 E, const u32 H, u32* __restrict__ habund) {
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
            if (lo < H && lo < T.toff[at[x] + 1] && T.tq[lo] == mine) atomicMax(&habund[lo], q_abund[e0 + i]);   // (max: an entry listed twice)
        }
    }
}

// chunks of 64 values a lane has in flight in a pass of the select: a pass is a chain of dependent loads from L2, as a look-up is
constexpr u32 kSelectChunks = 4;

// Twice the median of vals[0 .. n) (n >= 1), for the whole wave: v(k1) + v(k2), k1 = (n - 1) / 2 and k2 = n / 2 counted from 0 in
// ascending order.  Up to 64 values are ranked in registers; more are selected by four passes over 8-bit digits from the top
// with the wave's 256-bin histogram `hist` in LDS, and the upper value, when it is another one, is the smallest above the lower.
__device__ inline u64 gather_median2(const u32* vals, const u32 n, u32* hist, const u32 lane) {
    const u32 k1 = (n - 1) / 2, k2 = n / 2;
    if (n <= 64) {
        const bool has = lane < n;
        const u32 a = has ? load_u32(&vals[lane]) : 0;
        u32 rank = 0;
        for (u32 j = 0; j < n; ++j) {   // (the same trips for every lane)
            const u32 aj = (u32)__shfl((int)a, (int)j);
            rank += (aj < a || (aj == a && j < lane)) ? 1u : 0u;
        }
        const unsigned long long b1 = __ballot(has && rank == k1), b2 = __ballot(has && rank == k2);
        const u32 v1 = (u32)__shfl((int)a, __ffsll((long long)b1) - 1), v2 = (u32)__shfl((int)a, __ffsll((long long)b2) - 1);
        return (u64)v1 + v2;
    }
    u32 prefix = 0, r = k1, eq = n;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const u32 above = pass ? 0xFFFFFFFFu << (shift + 8) : 0u;   // the digits already chosen
#pragma unroll
        for (int b = 0; b < 4; ++b) hist[4 * lane + b] = 0;
        query_group_sync<true>();
        for (u32 i0 = 0; i0 < n; i0 += 64 * kSelectChunks) {   // (the same trips for every lane)
            u32 v[kSelectChunks];
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x) v[x] = i0 + 64 * x + lane < n ? load_u32(&vals[i0 + 64 * x + lane]) : 0;
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x)
                if (i0 + 64 * x + lane < n && (v[x] & above) == prefix) atomicAdd(&hist[(v[x] >> shift) & 255u], 1u);
        }
        query_group_sync<true>();
        u32 c[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = hist[4 * lane + b];
        const u32 mine = c[0] + c[1] + c[2] + c[3];
        u32 incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u32 o = (u32)__shfl_up((int)incl, d);
            if (lane >= (u32)d) incl += o;
        }
        const unsigned long long past = __ballot(incl > r);   // (not empty: the bins hold more than r values)
        const int L = past ? __ffsll((long long)past) - 1 : 63;
        u32 rr = r - (incl - mine), digit = 4 * lane, cnt = c[0];
        if (rr >= c[0]) { rr -= c[0]; ++digit; cnt = c[1];
            if (rr >= c[1]) { rr -= c[1]; ++digit; cnt = c[2];
                if (rr >= c[2]) { rr -= c[2]; ++digit; cnt = c[3]; } } }
        prefix |= (u32)__shfl((int)digit, L) << shift;
        r = (u32)__shfl((int)rr, L);
        eq = (u32)__shfl((int)cnt, L);
        query_group_sync<true>();   // (the bins are read before the next pass clears them)
    }
    const u32 v1 = prefix;   // r = how many of the eq values equal to v1 lie before rank k1
    if (k2 == k1 || r + 1 < eq) return 2ull * v1;
    u32 next = 0xFFFFFFFFu;   // rank k2 is the smallest value above v1 (there is one: k2 < n)
    for (u32 i0 = 0; i0 < n; i0 += 64 * kSelectChunks) {
        u32 v[kSelectChunks];
#pragma unroll
        for (u32 x = 0; x < kSelectChunks; ++x) v[x] = i0 + 64 * x + lane < n ? load_u32(&vals[i0 + 64 * x + lane]) : 0;   // (0 is never above v1)
#pragma unroll
        for (u32 x = 0; x < kSelectChunks; ++x)
            if (v[x] > v1 && v[x] < next) next = v[x];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) next = min(next, (u32)__shfl_xor((int)next, d));
    return (u64)v1 + next;
}

// what ONE wave does with query `tag` of the tile behind the counts of a round; kW: the weighted row (A and the wave's hist are set)
template <bool kW>
__device__ inline void gather_take(const GRound& R, const GAbund* A, u32* hist, const u32 tag, const u32 lane) {
    if (load_u32(&R.qdone[tag])) return;
    const unsigned long long w = load_u64(&R.best[tag]);
    if (w == 0) {   // nobody offered: nothing covers min_hashes of what is left
        if (lane == 0) { R.qdone[tag] = 1; atomicAdd(&R.ctrl[kLiveQ], ~0ull); }
        return;
    }
    const u32 u = (u32)(w >> 32), c = ~(u32)w;
    if (c >= R.n_cand) return;   // (never: an offer names its candidate)
    const u64 base = R.cbase[c];
    const u32 len = R.covl[c];
    u64 sum = 0, sq_lo = 0, sq_hi = 0, median2 = 0;
    if (kW) {
        // the alive slots before they are cleared: their abundances summed, and compacted to the front of the segment, which
        // nobody reads after this take — an abundance goes to an entry at or before its own slot's, which the wave has read by then
        // (every trip loads its kSelectChunks chunks before it stores)
        u32 n = 0;
        for (u32 i0 = 0; i0 < len; i0 += 64 * kSelectChunks) {   // (the same trips for every lane; the loads of a step together)
            u32 h[kSelectChunks], a[kSelectChunks];
            bool on[kSelectChunks];
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x) h[x] = i0 + 64 * x + lane < len ? R.seg[base + i0 + 64 * x + lane] : 0;
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x) on[x] = i0 + 64 * x + lane < len && ((load_u32(&R.alive[h[x] >> 5]) >> (h[x] & 31)) & 1u);
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x) a[x] = on[x] ? A->habund[h[x]] : 0;
#pragma unroll
            for (u32 x = 0; x < kSelectChunks; ++x) {   // (a slot's bit is cleared by its own lane alone: the words read above hold for it)
                const unsigned long long b = __ballot(on[x]);
                if (on[x]) {
                    const u64 aa = (u64)a[x] * a[x];
                    atomicAnd(&R.alive[h[x] >> 5], ~(1u << (h[x] & 31)));
                    sum += a[x];
                    sq_lo += aa;
                    sq_hi += sq_lo < aa;
                    A->vals[base + n + (u32)__popcll(b & ((1ull << lane) - 1))] = a[x];
                }
                n += (u32)__popcll(b);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");   // the abundances are in memory before the wave reads them back
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const u64 lo = shfl_down_u64(sq_lo, d), hi = shfl_down_u64(sq_hi, d);
            sum += shfl_down_u64(sum, d);
            sq_lo += lo;
            sq_hi += hi + (sq_lo < lo);
        }
        if (n) median2 = gather_median2(A->vals + base, n, hist, lane);   // (n = u >= min_hashes >= 1)
    } else {
        for (u32 i = lane; i < len; i += 64) {
            const u32 h = R.seg[base + i];
            const u32 bit = 1u << (h & 31);
            if (load_u32(&R.alive[h >> 5]) & bit) atomicAnd(&R.alive[h >> 5], ~bit);
        }
    }
    if (lane == 0) {
        const u32 rank = R.qrank[tag] + 1, rem = R.qrem[tag] - u;
        const unsigned long long at = atomicAdd(&R.ctrl[kRows], 1ull);
        if (kW) {
            const unsigned long long found = A->qwfound[tag] + sum;
            A->qwfound[tag] = found;
            if (at < R.rows_cap) A->rows[at] = ksp_gather_wrow{R.q0 + tag, rank, (u32)R.ckey[c], len, u, rem, sum, found, sq_lo, sq_hi, median2};
        } else if (at < R.rows_cap) {
            R.rows[at] = ksp_gather_row{R.q0 + tag, rank, (u32)R.ckey[c], len, u, rem};
        }
        R.qrank[tag] = rank;
        R.qrem[tag] = rem;
        R.best[tag] = 0;
        R.cdead[c] = 1;
        if (R.max_matches && rank >= R.max_matches) { R.qdone[tag] = 1; atomicAdd(&R.ctrl[kLiveQ], ~0ull); }
    }
}

// The counts of a round: workgroups [0, short_groups) take the short list, a wave per candidate; the others the long list, a
// workgroup per candidate.  Returns at once when no query is live.
__global__ __launch_bounds__(kThreads) void k_gather_count(const GRound R, const u32* __restrict__ list0, const u32 n0, const u32 short_groups,
                                                           const u32* __restrict__ list1, const u32 n1) {
    __shared__ u32 s_u;
    const bool go = load_u64(&R.ctrl[kLiveQ]) != 0;   // (no kernel of a round's counts changes it)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        R.ctrl[kGo] = go;
        if (go) R.ctrl[kRounds] += 1;
    }
    if (!go) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x < short_groups) {
        for (u64 i = (u64)blockIdx.x * kWaves + wave; i < n0; i += (u64)short_groups * kWaves) {
            const u32 c = list0[i];
            if (!gather_is_live(R, c)) continue;   // (the whole wave)
            const u32 u = gather_alive(R, c, 0, 64, lane);
            if (lane == 0) gather_offer(R, c, u);
        }
    } else {
        const u32 long_groups = gridDim.x - short_groups;
        for (u64 i = blockIdx.x - short_groups; i < n1; i += long_groups) {
            const u32 c = list1[i];
            if (!gather_is_live(R, c)) continue;   // (the whole workgroup)
            if (threadIdx.x == 0) s_u = 0;
            __syncthreads();
            const u32 u = gather_alive(R, c, wave * 64, kThreads, lane);
            if (lane == 0 && u) atomicAdd(&s_u, u);
            __syncthreads();
            if (threadIdx.x == 0) gather_offer(R, c, s_u);
            __syncthreads();
        }
    }
}

// The takes of a round: a wave per query of the tile.
__global__ __launch_bounds__(kThreads) void k_gather_take(const GRound R) {
    if (load_u64(&R.ctrl[kGo]) == 0) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 tag = (u64)blockIdx.x * kWaves + wave; tag < R.nq; tag += (u64)gridDim.x * kWaves) gather_take<false>(R, nullptr, nullptr, (u32)tag, lane);
}

// the same with the weighted rows
__global__ __launch_bounds__(kThreads) void k_gather_take_w(const GRound R, const GAbund A) {
    __shared__ u32 s_hist[kWaves][256];
    if (load_u64(&R.ctrl[kGo]) == 0) return;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 tag = (u64)blockIdx.x * kWaves + wave; tag < R.nq; tag += (u64)gridDim.x * kWaves) gather_take<true>(R, &A, s_hist[wave], (u32)tag, lane);
}

// The remaining rounds by ONE workgroup: the same counts and takes, separated by __syncthreads() and not by dispatches.  A round
// with a live query takes a candidate or finishes every query, so `bound` = the live candidates + 1 rounds suffice.  Hand-over:
// the queries it finds unfinished must be the device's count of them (out[2] = 1 otherwise, and nothing runs).  out[0] = the
// rounds that ran, out[1] = the queries still live (0 unless the bound was hit, which the host reports).
template <bool kW>
__device__ inline void gather_tail(const GRound& R, const GAbund* A, u32* hist, const u32* __restrict__ list0, const u32 n0, const u32* __restrict__ list1, const u32 n1,
                                   const u32 bound, u32* __restrict__ out) {
    __shared__ u32 s_live;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_live = 0;
    __syncthreads();
    u32 mine = 0;
    for (u32 j = threadIdx.x; j < R.nq; j += kTailThreads) mine += !load_u32(&R.qdone[j]);
    if (mine) atomicAdd(&s_live, mine);
    __syncthreads();
    u32 live = s_live, rounds = 0;
    const bool handed = live == (u32)load_u64(&R.ctrl[kLiveQ]);
    __syncthreads();
    for (u32 it = 0; handed && it < bound && live; ++it) {
        for (u32 i = wave; i < n0 + n1; i += kTailWaves) {
            const u32 c = i < n0 ? list0[i] : list1[i - n0];
            if (!gather_is_live(R, c)) continue;   // (the whole wave)
            const u32 u = gather_alive(R, c, 0, 64, lane);
            if (lane == 0) gather_offer(R, c, u);
        }
        __threadfence();
        __syncthreads();   // every offer of this round is made
        for (u32 tag = wave; tag < R.nq; tag += kTailWaves) gather_take<kW>(R, A, hist, tag, lane);
        __threadfence();
        __syncthreads();   // every take of this round is made
        if (threadIdx.x == 0) s_live = (u32)load_u64(&R.ctrl[kLiveQ]);
        __syncthreads();
        live = s_live;
        ++rounds;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        R.ctrl[kRounds] += rounds;
        out[0] = rounds;
        out[1] = live;
        out[2] = handed ? 0 : 1;
    }
}

__global__ __launch_bounds__(kTailThreads) void k_gather_tail(const GRound R, const u32* __restrict__ list0, const u32 n0, const u32* __restrict__ list1, const u32 n1,
                                                              const u32 bound, u32* __restrict__ out) {
    gather_tail<false>(R, nullptr, nullptr, list0, n0, list1, n1, bound, out);
}

__global__ __launch_bounds__(kTailThreads) void k_gather_tail_w(const GRound R, const GAbund A, const u32* __restrict__ list0, const u32 n0, const u32* __restrict__ list1,
                                                                const u32 n1, const u32 bound, u32* __restrict__ out) {
    __shared__ u32 s_hist[kTailWaves][256];
    gather_tail<true>(R, &A, s_hist[threadIdx.x >> 6], list0, n0, list1, n1, bound, out);
}

// per query of the tile: nothing found yet, everything left; every query is live (the device's words were zeroed before)
__global__ void k_gather_init(const u64* __restrict__ q_off, const GRound R) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= R.nq) return;
    if (j == 0) R.ctrl[kLiveQ] = R.nq;
    R.best[j] = 0;
    R.qrank[j] = 0;
    R.qdone[j] = 0;
    R.qrem[j] = (u32)(q_off[R.q0 + j + 1] - q_off[R.q0 + j]);   // (a tile has fewer than 2^31 entries)
}

// The live candidates of `in` (in == NULL: of all candidates), split by segment length when `out1` is given: one append per wave.
__global__ __launch_bounds__(kThreads) void k_gather_live(const GRound R, const u32* __restrict__ in, const u32 n, const u64 long_seg, const bool split, u32* __restrict__ out0,
                                                          u32* __restrict__ out1, const int word0) {
    const u32 lane = threadIdx.x & 63;
    const u64 span = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += span) {   // (the same trips for every lane of the wave)
        const u64 i = base + threadIdx.x;
        const u32 c = i < n ? (in ? in[i] : (u32)i) : kNone;
        const bool keep = i < n && gather_is_live(R, c);
        const bool is_long = keep && split && (u64)R.covl[c] >= long_seg;
#pragma unroll
        for (int cls = 0; cls < 2; ++cls) {
            const unsigned long long b = __ballot(keep && is_long == (cls == 1));
            if (!b) continue;
            unsigned long long at = 0;
            const int src = __ffsll((long long)b) - 1;
            if (lane == (u32)src) at = atomicAdd(&R.ctrl[word0 + cls], (unsigned long long)__popcll(b));
            const u32 pos = (u32)__shfl((int)(u32)at, src) + (u32)__popcll(b & ((1ull << lane) - 1));
            if (keep && is_long == (cls == 1) && pos < R.n_cand) (cls ? out1 : out0)[pos] = c;
        }
    }
}

// the tile's rows `in`, of either kind, into (query, rank) order: qoff[] = the exclusive scan of the queries' row counts
template <class Row>
__global__ void k_gather_rows(const GRound R, const Row* __restrict__ in, const u32 n_rows, const u32* __restrict__ qoff, Row* __restrict__ sorted) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows; i += (u64)gridDim.x * blockDim.x) {
        const Row r = in[i];
        const u32 tag = r.query - R.q0;
        if (tag >= R.nq || r.rank == 0) continue;
        const u64 at = (u64)qoff[tag] + r.rank - 1;
        if (at < n_rows) sorted[at] = r;
    }
}

struct AsU64 {
    __host__ __device__ u64 operator()(const u32 v) const { return v; }
};

// what all entry points refuse before anything is allocated
int check_gather_args(const char* who, const void* db_keys, const u64* db_off, const u32 n_db, const void* q_keys, const u64* q_off, const u32 n_q, const u32 min_hashes,
                      const void* n_rows) {
    if (!db_keys || !db_off || !q_keys || !q_off || !n_rows) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_db == 0 || n_q == 0) { ksp::set_error(std::string(who) + ": no database source or no query"); return KSP_E_ARG; }
    if (min_hashes == 0) { ksp::set_error(std::string(who) + ": min_hashes is 1 or more"); return KSP_E_ARG; }
    if ((u64)n_db + n_q > 0xFFFFFFFEull) { ksp::set_error(std::string(who) + ": more than 2^32 - 2 sources"); return KSP_E_LIMIT; }   // (from the counts alone)
    if (const int rc = check_offsets(who, "database", db_off, n_db)) return rc;
    return check_offsets(who, "query", q_off, n_q);
}

struct GatherSwitches {
    u64 tile = 0, long_run = 0, list_cap = 0, long_seg = 0, tail = 0, tail_cands = 0;
};

// the environment's switches, refused before a device is chosen
int read_switches(const char* who, GatherSwitches& W) {
    int rc = KSP_OK;
    if ((rc = env_number(who, "KSP_QUERY_TILE", kTileMax, 1, kTileMax, &W.tile)) || (rc = env_number(who, "KSP_QUERY_LONG_RUN", KSP_QUERY_LONG_RUN, 1, ~0ull, &W.long_run)) ||
        (rc = env_number(who, "KSP_QUERY_LIST", kListMax, 1, kListMax, &W.list_cap)) || (rc = env_number(who, "KSP_GATHER_LONG_SEG", KSP_GATHER_LONG_SEG, 1, 0xFFFFFFFFull, &W.long_seg)) ||
        (rc = env_number(who, "KSP_GATHER_TAIL", 1, 0, 1, &W.tail)) || (rc = env_number(who, "KSP_GATHER_TAIL_CANDS", KSP_GATHER_TAIL_CANDS, 0, KSP_GATHER_TAIL_CANDS_MAX, &W.tail_cands)))
        return rc;
    return KSP_OK;
}

// One tile of queries: its table, what the steps found, and its own arrays, which go back to the device when the tile is done
template <class Row>
struct GatherTile {
    u32 q0 = 0, nq = 0, E = 0, U = 0, H = 0, n_cand = 0;
    u64 e0 = 0, n_fill[2] = {0, 0}, n_slots = 0, rows_cap = 0, found = 0;
    QTable T;
    GSweep P;
    GRound R;
    GAbund AB;
    ksp::DeviceArena mem;   // of the arrays below
    // the sorted candidates (key 8, overlap 4, base 8, dead 4, two live lists 2 x 2 x 4) and the sort's scratch
    u64 *ckey = nullptr, *cbase = nullptr;
    u32 *covl = nullptr, *cdead = nullptr, *live[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    void* tmp2 = nullptr;
    size_t tb2 = 0;
    // when the slots are known: 4 per slot, a bit per holder, weighted 4 per holder; the rows as found and by (query, rank)
    u32 *seg = nullptr, *alive = nullptr, *habund = nullptr;
    Row *rows = nullptr, *sorted = nullptr;
};

// One gather call on the CURRENT device (weighted: 7q): what it is given, what it holds whatever the tiles find,
// and its phases as steps.  The arguments have passed check_gather_args and read_switches.  The rows go to d_rows (room for
// `capacity`) or, when h_rows is given, to the host vector.  Row = ksp_gather_wrow: the weighted call, d_q_abund beside the
// query keys; Row = ksp_gather_row: d_q_abund is not read.
template <class Row>
struct GatherCall {
    static constexpr bool kW = std::is_same<Row, ksp_gather_wrow>::value;
    typedef GatherTile<Row> Tile;

    const char* who;
    GatherSwitches W;
    const u64 *d_db_keys, *h_db_off;
    u32 n_db;
    const u64* d_q_keys;
    const u32* d_q_abund;
    const u64* h_q_off;
    u32 n_q, min_hashes, max_matches;
    Row* d_rows;
    u64 capacity;
    std::vector<Row>* h_rows;
    // (an aggregate: the members above are the call's arguments, in this order)
    ksp::WorkgroupCap G;
    ksp::DeviceArena A;
    ksp::Events<5> ev;   // of a tile: table | candidates | fill | rounds
    u32 n_tiles = 0;
    std::vector<u32> probes[2];   // [0] short, [1] long
    u64 *d_db_off = nullptr, *d_q_off = nullptr;
    u32 *d_list[2] = {nullptr, nullptr}, *d_fill[2] = {nullptr, nullptr};   // the sources of a sweep; those of them that have a candidate
    u32 *qrank = nullptr, *qrem = nullptr, *qdone = nullptr, *qoff = nullptr, *d_out = nullptr;   // per query of a tile; the tail's report
    unsigned long long *ctrl = nullptr, *best = nullptr, *qwfound = nullptr;   // (qwfound: weighted only)
    unsigned long long h_ctrl[kCtrlWords] = {};
    u64* cand_key = nullptr;   // the candidates as the sweep found them; they grow when a tile finds more
    u32* cand_ovl = nullptr;
    u64 cand_cap = 0;
    QTableBufs B;
    ksp_gather_stats S = {};
    u64 rows_done = 0;

    // ---- what the call holds whatever the tiles find, sized and checked first: 8 per source (offsets), 8 per source with entries
    // (its list and the list of those with a candidate), 24 per query of a tile, the table, the first candidate buffer, the scratch
    int setup() {
        int rc = KSP_OK;
        u64 e_max = 0;
        if ((rc = query_tiles(who, h_q_off, n_q, W.tile, &n_tiles, &e_max))) return rc;
        if ((rc = ksp::workgroup_cap("KSP_GATHER_MAX_WORKGROUPS", who, G))) return rc;
        query_split_sources(h_db_off, n_db, W.long_run, 0, probes);
        S.n_db = n_db; S.n_q = n_q; S.db_entries = h_db_off[n_db]; S.q_entries = h_q_off[n_q];
        S.tile = (u32)W.tile; S.long_seg = W.long_seg; S.tail_cands = W.tail ? W.tail_cands : 0; S.min_hashes = min_hashes; S.max_matches = max_matches;
        size_t tb_rows = 0;
        B.e_max = e_max;
        if ((rc = query_table_scratch(e_max, &B.tb))) return rc;
        KSP_HIP(rocprim::exclusive_scan(nullptr, tb_rows, (u32*)nullptr, (u32*)nullptr, 0u, (size_t)kTileMax, rocprim::plus<u32>(), (hipStream_t) nullptr));
        B.tb = std::max<size_t>(std::max(B.tb, tb_rows), 8);
        cand_cap = std::max<u64>(KSP_GATHER_FIRST_CANDS, 4ull * n_db);
        if ((rc = ksp::device_fits(who, 8ull * ((u64)n_db + n_q + 2) + 8ull * (probes[0].size() + probes[1].size()) + (kW ? 32ull : 24ull) * kTileMax + B.bytes() + 12 * cand_cap + B.tb + 256,
                                   kW ? "8 per source, 8 per source with entries, 40 per entry of the largest query tile, its directory, the candidates, the sort's scratch, 8 per query of a tile"
                                      : "8 per source, 8 per source with entries, 40 per entry of the largest query tile, its directory, the candidates, the sort's scratch")))
            return rc;
        if ((rc = query_upload_front(A, h_db_off, n_db, h_q_off, n_q, probes, &d_db_off, &d_q_off, d_list)) || (rc = A.alloc(&ctrl, (size_t)kCtrlWords)) || (rc = A.alloc(&d_out, 4)))
            return rc;
        for (int c = 0; c < 2; ++c)
            if (!probes[c].empty() && (rc = A.alloc(&d_fill[c], probes[c].size()))) return rc;
        if ((rc = A.alloc(&best, (size_t)kTileMax)) || (rc = A.alloc(&qrank, (size_t)kTileMax)) || (rc = A.alloc(&qrem, (size_t)kTileMax)) || (rc = A.alloc(&qdone, (size_t)kTileMax)) ||
            (rc = A.alloc(&qoff, (size_t)kTileMax)))
            return rc;
        if constexpr (kW)
            if ((rc = A.alloc(&qwfound, (size_t)kTileMax))) return rc;
        if ((rc = A.alloc(&cand_key, (size_t)cand_cap)) || (rc = A.alloc(&cand_ovl, (size_t)cand_cap))) return rc;
        if (e_max && ((rc = query_table_alloc(A, B)) || (rc = A.alloc_bytes(&B.tmp, B.tb)))) return rc;
        return ev.create();
    }

    // ---- the candidates: every source against this tile; once more with a larger buffer when it found more than fit
    int candidates(Tile& t) {
        int rc = KSP_OK;
        GSweep& P = t.P;
        std::memset(&P, 0, sizeof P);
        P.db_keys = d_db_keys; P.db_off = d_db_off; P.list_cap = (u32)W.list_cap; P.min_hashes = min_hashes; P.ctrl = ctrl;
        for (int attempt = 0; attempt < 2; ++attempt) {
            KSP_HIP(hipMemsetAsync(ctrl, 0, sizeof h_ctrl, nullptr));
            P.cand_key = cand_key; P.cand_ovl = cand_ovl; P.cand_cap = cand_cap;
            if (!probes[0].empty()) {
                P.list = d_list[0]; P.n_list = (u32)probes[0].size(); P.fill_list = d_fill[0]; P.fill_word = kFill0;
                hipLaunchKernelGGL((k_gather_sweep<true, false>), dim3(G.grid_of(((u64)P.n_list + kWaves - 1) / kWaves)), dim3(kThreads), 0, nullptr, t.T, P);
            }
            if (!probes[1].empty()) {
                P.list = d_list[1]; P.n_list = (u32)probes[1].size(); P.fill_list = d_fill[1]; P.fill_word = kFill1;
                hipLaunchKernelGGL((k_gather_sweep<false, false>), dim3(G.grid_of(P.n_list)), dim3(kThreads), 0, nullptr, t.T, P);
            }
            KSP_HIP(hipGetLastError());
            KSP_HIP(hipMemcpy(h_ctrl, ctrl, sizeof h_ctrl, hipMemcpyDeviceToHost));
            if (h_ctrl[kCands] <= cand_cap) break;
            if (attempt == 1) { ksp::set_error(std::string(who) + ": the second sweep found more candidates than the first"); return KSP_E_HIP; }
            if (h_ctrl[kCands] >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 candidates or more in a query tile (lower KSP_QUERY_TILE)"); return KSP_E_LIMIT; }
            KSP_HIP(A.release(cand_key));
            KSP_HIP(A.release(cand_ovl));
            cand_key = nullptr; cand_ovl = nullptr;
            cand_cap = h_ctrl[kCands];
            if ((rc = ksp::device_fits(who, 12 * cand_cap, "the candidates of a query tile"))) return rc;
            if ((rc = A.alloc(&cand_key, (size_t)cand_cap)) || (rc = A.alloc(&cand_ovl, (size_t)cand_cap))) return rc;
        }
        t.n_cand = (u32)h_ctrl[kCands];
        t.n_fill[0] = h_ctrl[kFill0]; t.n_fill[1] = h_ctrl[kFill1];
        if (t.n_fill[0] > probes[0].size() || t.n_fill[1] > probes[1].size()) { ksp::set_error(std::string(who) + ": more sources with a candidate than sources"); return KSP_E_HIP; }
        S.candidates += t.n_cand; S.dropped += h_ctrl[kDropped]; S.table_keys += t.U; S.table_holders += t.H; ++S.passes;
        return KSP_OK;
    }

    // ---- the candidates sorted by (query, source), a segment for each by the scan of the overlaps, the slots of all of them
    int sort_candidates(Tile& t) {
        int rc = KSP_OK;
        const u32 n_cand = t.n_cand;
        size_t tb_sort = 0, tb_scan = 0;
        const auto ovl64 = [](const u32* p) { return rocprim::make_transform_iterator(p, AsU64()); };
        KSP_HIP(rocprim::radix_sort_pairs(nullptr, tb_sort, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)n_cand, 0, 44, (hipStream_t) nullptr));
        KSP_HIP(rocprim::exclusive_scan(nullptr, tb_scan, ovl64(nullptr), (u64*)nullptr, (u64)0, (size_t)n_cand + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        t.tb2 = std::max<size_t>(std::max(tb_sort, tb_scan), 8);
        if ((rc = ksp::device_fits(who, 40ull * ((u64)n_cand + 1) + t.tb2, "40 per candidate of a query tile, the sort's scratch"))) return rc;
        if ((rc = t.mem.alloc(&t.ckey, (size_t)n_cand)) || (rc = t.mem.alloc(&t.covl, (size_t)n_cand + 1)) || (rc = t.mem.alloc(&t.cbase, (size_t)n_cand + 1)) ||
            (rc = t.mem.alloc(&t.cdead, (size_t)n_cand)) || (rc = t.mem.alloc_bytes(&t.tmp2, t.tb2)))
            return rc;
        for (int b = 0; b < 2; ++b)
            for (int c = 0; c < 2; ++c)
                if ((rc = t.mem.alloc(&t.live[b][c], (size_t)n_cand))) return rc;
        size_t b = t.tb2;
        KSP_HIP(rocprim::radix_sort_pairs(t.tmp2, b, (const u64*)cand_key, t.ckey, (const u32*)cand_ovl, t.covl, (size_t)n_cand, 0, 44, (hipStream_t) nullptr));
        KSP_HIP(hipMemsetAsync(t.covl + n_cand, 0, 4, nullptr));
        KSP_HIP(hipMemsetAsync(t.cdead, 0, (size_t)n_cand * 4, nullptr));
        b = t.tb2;
        KSP_HIP(rocprim::exclusive_scan(t.tmp2, b, ovl64(t.covl), t.cbase, (u64)0, (size_t)n_cand + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        KSP_HIP(hipMemcpy(&t.n_slots, t.cbase + n_cand, 8, hipMemcpyDeviceToHost));
        if (t.n_slots >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": match segments of 2^32 - 1 slots or more in a query tile (lower KSP_QUERY_TILE)"); return KSP_E_LIMIT; }
        if (t.n_slots < (u64)n_cand * min_hashes) { ksp::set_error(std::string(who) + ": the segments are shorter than their candidates' overlaps"); return KSP_E_HIP; }
        S.slots += t.n_slots;
        return KSP_OK;
    }

    // ---- the segments: the sources that have a candidate once more
    int segments(Tile& t) {
        int rc = KSP_OK;
        const u64 alive_words = ((u64)t.H + 31) / 32;
        // a row removes min_hashes or more of its query, and a candidate is taken once
        t.rows_cap = std::min<u64>(std::min<u64>(t.n_cand, (u64)t.E / min_hashes), max_matches ? (u64)t.nq * max_matches : ~0ull);
        if ((rc = ksp::device_fits(who, 4 * t.n_slots + 4 * alive_words + 2 * sizeof(Row) * t.rows_cap + (kW ? 4ull * t.H : 0) + 64,
                                   kW ? "4 per matched hash of a candidate, a bit per query hash, 4 per holder of the query table, 128 per possible row"
                                      : "4 per matched hash of a candidate, a bit per query hash, 48 per possible row")))
            return rc;
        if ((rc = t.mem.alloc(&t.seg, (size_t)t.n_slots)) || (rc = t.mem.alloc(&t.alive, (size_t)alive_words)) || (rc = t.mem.alloc(&t.rows, (size_t)t.rows_cap + 1)) ||
            (rc = t.mem.alloc(&t.sorted, (size_t)t.rows_cap + 1)))
            return rc;
        KSP_HIP(hipMemsetAsync(t.alive, 0xFF, (size_t)alive_words * 4, nullptr));
        if constexpr (kW) {   // the abundance of every (hash, query) of the tile at its holder slot
            if ((rc = t.mem.alloc(&t.habund, (size_t)t.H))) return rc;
            KSP_HIP(hipMemsetAsync(t.habund, 0, (size_t)t.H * 4, nullptr));
            KSP_HIP(hipMemsetAsync(qwfound, 0, (size_t)kTileMax * 8, nullptr));
            hipLaunchKernelGGL(k_gather_habund, dim3(G.grid_of(((u64)t.E + (u64)kThreads * kProbeKeys - 1) / ((u64)kThreads * kProbeKeys))), dim3(kThreads), 0, nullptr, t.T, d_q_keys,
                               d_q_abund, (const u32*)B.tag, t.e0, t.E, t.H, t.habund);
            KSP_HIP(hipGetLastError());
        }
        GSweep& P = t.P;
        P.ckey = t.ckey; P.cbase = t.cbase; P.n_cand = t.n_cand; P.seg = t.seg; P.n_slots = (u32)t.n_slots;
        if (t.n_fill[0]) {
            P.list = d_fill[0]; P.n_list = (u32)t.n_fill[0];
            hipLaunchKernelGGL((k_gather_sweep<true, true>), dim3(G.grid_of(((u64)P.n_list + kWaves - 1) / kWaves)), dim3(kThreads), 0, nullptr, t.T, P);
        }
        if (t.n_fill[1]) {
            P.list = d_fill[1]; P.n_list = (u32)t.n_fill[1];
            hipLaunchKernelGGL((k_gather_sweep<false, true>), dim3(G.grid_of(P.n_list)), dim3(kThreads), 0, nullptr, t.T, P);
        }
        KSP_HIP(hipGetLastError());
        return KSP_OK;
    }

    // the takes of a round, by the kernel of the row type: a wave per query of the tile
    void launch_take(const Tile& t) {
        const dim3 grid(G.grid_of(((u64)t.nq + kWaves - 1) / kWaves));
        if constexpr (kW) hipLaunchKernelGGL(k_gather_take_w, grid, dim3(kThreads), 0, nullptr, t.R, t.AB);
        else hipLaunchKernelGGL(k_gather_take, grid, dim3(kThreads), 0, nullptr, t.R);
    }

    // the remaining rounds over the live lists `cur`, by the tail kernel of the row type: one workgroup
    void launch_tail(const Tile& t, const int cur, const u64 (&n_live)[2]) {
        const u32* const list[2] = {t.live[cur][0], t.live[cur][1]};
        const u32 bound = (u32)(n_live[0] + n_live[1]) + 1;
        if constexpr (kW)
            hipLaunchKernelGGL(k_gather_tail_w, dim3(1), dim3(kTailThreads), 0, nullptr, t.R, t.AB, list[0], (u32)n_live[0], list[1], (u32)n_live[1], bound, d_out);
        else
            hipLaunchKernelGGL(k_gather_tail, dim3(1), dim3(kTailThreads), 0, nullptr, t.R, list[0], (u32)n_live[0], list[1], (u32)n_live[1], bound, d_out);
    }

    // ---- the rounds: every query live, every candidate in the live lists; batches of rounds until no query is live, or the tail
    int rounds(Tile& t) {
        t.R = GRound{t.ckey, t.covl, t.cbase, t.seg, t.alive, t.cdead, best, qrank, qrem, qdone, t.n_cand, t.nq, t.q0, min_hashes, max_matches, nullptr, (u32)t.rows_cap, ctrl};
        t.AB = GAbund{t.habund, t.seg, qwfound, nullptr};
        if constexpr (kW) t.AB.rows = t.rows;
        else t.R.rows = t.rows;
        const GRound& R = t.R;
        const unsigned gq = (unsigned)(((u64)t.nq + 255) / 256), gc = G.grid_of(((u64)t.n_cand + kThreads - 1) / kThreads);
        u64 n_live[2] = {0, 0};
        int cur = 0;
        bool in_tail = false;
        KSP_HIP(hipMemsetAsync(ctrl, 0, sizeof h_ctrl, nullptr));
        hipLaunchKernelGGL(k_gather_init, dim3(gq), dim3(256), 0, nullptr, (const u64*)d_q_off, R);
        hipLaunchKernelGGL(k_gather_live, dim3(gc), dim3(kThreads), 0, nullptr, R, (const u32*)nullptr, t.n_cand, W.long_seg, true, t.live[cur][0], t.live[cur][1], (int)kKept0);
        KSP_HIP(hipGetLastError());
        KSP_HIP(hipMemcpy(h_ctrl, ctrl, sizeof h_ctrl, hipMemcpyDeviceToHost));
        n_live[0] = h_ctrl[kKept0]; n_live[1] = h_ctrl[kKept1];
        if (n_live[0] + n_live[1] != t.n_cand) { ksp::set_error(std::string(who) + ": the first live lists do not hold every candidate"); return KSP_E_HIP; }
        const u64 max_batches = (u64)t.n_cand / KSP_GATHER_BATCH + 2;   // a round with a live query takes a candidate or finishes every query
        u64 batches = 0;
        while (h_ctrl[kLiveQ]) {
            const u64 n_both = n_live[0] + n_live[1];
            if (W.tail && n_both <= W.tail_cands) {
                u32 h_out[4] = {0, 0, 0, 0};
                launch_tail(t, cur, n_live);
                KSP_HIP(hipGetLastError());
                KSP_HIP(hipMemcpy(h_out, d_out, 12, hipMemcpyDeviceToHost));
                if (h_out[2]) { ksp::set_error(std::string(who) + ": the tail's count of live queries does not match the batches'"); return KSP_E_HIP; }
                if (h_out[1]) { ksp::set_error(std::string(who) + ": the tail left " + std::to_string(h_out[1]) + " queries live after " + std::to_string(h_out[0]) + " rounds"); return KSP_E_HIP; }
                S.tail_rounds += h_out[0];
                S.live_at_tail += n_both;
                in_tail = true;
                break;
            }
            if (++batches > max_batches) { ksp::set_error(std::string(who) + ": more than " + std::to_string(max_batches) + " batches of rounds"); return KSP_E_HIP; }
            const unsigned g0 = G.grid_of((n_live[0] + kWaves - 1) / kWaves), g1 = G.grid_of(n_live[1]);
            for (u32 r = 0; r < KSP_GATHER_BATCH; ++r) {
                hipLaunchKernelGGL(k_gather_count, dim3(g0 + g1), dim3(kThreads), 0, nullptr, R, (const u32*)t.live[cur][0], (u32)n_live[0], (u32)g0, (const u32*)t.live[cur][1], (u32)n_live[1]);
                launch_take(t);
            }
            // the dead leave the lists
            KSP_HIP(hipMemsetAsync(&ctrl[kKept0], 0, 16, nullptr));
            for (int c = 0; c < 2; ++c)
                if (n_live[c])
                    hipLaunchKernelGGL(k_gather_live, dim3(G.grid_of((n_live[c] + kThreads - 1) / kThreads)), dim3(kThreads), 0, nullptr, R, (const u32*)t.live[cur][c], (u32)n_live[c],
                                       W.long_seg, false, t.live[cur ^ 1][c], (u32*)nullptr, (int)kKept0 + c);
            KSP_HIP(hipGetLastError());
            KSP_HIP(hipMemcpy(h_ctrl, ctrl, sizeof h_ctrl, hipMemcpyDeviceToHost));
            if (h_ctrl[kKept0] > n_live[0] || h_ctrl[kKept1] > n_live[1]) { ksp::set_error(std::string(who) + ": a compaction kept more candidates than its list holds"); return KSP_E_HIP; }
            n_live[0] = h_ctrl[kKept0]; n_live[1] = h_ctrl[kKept1];
            cur ^= 1;
            ++S.batches;
        }
        if (in_tail) KSP_HIP(hipMemcpy(h_ctrl, ctrl, sizeof h_ctrl, hipMemcpyDeviceToHost));
        S.rounds += h_ctrl[kRounds]; S.fell_below += h_ctrl[kFell];
        t.found = h_ctrl[kRows];
        if (t.found > t.rows_cap) { ksp::set_error(std::string(who) + ": more rows than a tile can have"); return KSP_E_HIP; }
        return KSP_OK;
    }

    // ---- the tile's rows, by (query, rank), behind the rows of the tiles before it
    int emit_rows(Tile& t) {
        if (!t.found) return KSP_OK;
        size_t b = B.tb;
        KSP_HIP(rocprim::exclusive_scan(B.tmp, b, (const u32*)qrank, qoff, 0u, (size_t)t.nq, rocprim::plus<u32>(), (hipStream_t) nullptr));
        hipLaunchKernelGGL(k_gather_rows<Row>, dim3(G.grid_of((t.found + 255) / 256)), dim3(256), 0, nullptr, t.R, (const Row*)t.rows, (u32)t.found, (const u32*)qoff, t.sorted);
        KSP_HIP(hipGetLastError());
        if (h_rows) {
            const size_t at = h_rows->size();
            h_rows->resize(at + (size_t)t.found);
            KSP_HIP(hipMemcpy(h_rows->data() + at, t.sorted, (size_t)t.found * sizeof(Row), hipMemcpyDeviceToHost));
        } else if (rows_done < capacity) {
            KSP_HIP(hipMemcpyAsync(d_rows + rows_done, t.sorted, (size_t)std::min<u64>(t.found, capacity - rows_done) * sizeof(Row), hipMemcpyDeviceToDevice, nullptr));
        }
        rows_done += t.found;
        return KSP_OK;
    }

    // the tile has reached event `last`: the times between its events go to the phases' sums
    int add_times(const int last) {
        float* const phase[4] = {&S.ms_table, &S.ms_candidates, &S.ms_fill, &S.ms_rounds};
        KSP_HIP(hipEventSynchronize(ev[last]));
        for (int i = 0; i < last; ++i) {
            float ms = 0;
            KSP_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            *phase[i] += ms;
        }
        return KSP_OK;
    }

    // tile `index`: the steps between the event records that bound ms_table, ms_candidates, ms_fill and ms_rounds
    int run_tile(const u32 index) {
        int rc = KSP_OK;
        Tile t;
        t.q0 = (u32)((u64)index * W.tile);
        t.nq = (u32)(std::min<u64>((u64)t.q0 + W.tile, n_q) - t.q0);
        t.e0 = h_q_off[t.q0];
        t.E = (u32)(h_q_off[t.q0 + t.nq] - t.e0);
        if (t.E == 0) return KSP_OK;   // a tile of empty queries matches nothing
        KSP_HIP(hipEventRecord(ev[0], nullptr));
        if ((rc = query_table_build(who, G, B, d_q_keys, d_q_off, t.q0, t.nq, t.e0, t.E, &t.T, &t.U, &t.H))) return rc;
        KSP_HIP(hipEventRecord(ev[1], nullptr));
        if ((rc = candidates(t))) return rc;
        if (t.n_cand == 0) {   // nothing reaches min_hashes: no row for any query of the tile
            KSP_HIP(hipEventRecord(ev[2], nullptr));
            return add_times(2);
        }
        if ((rc = sort_candidates(t))) return rc;
        KSP_HIP(hipEventRecord(ev[2], nullptr));
        if ((rc = segments(t))) return rc;
        KSP_HIP(hipEventRecord(ev[3], nullptr));
        if ((rc = rounds(t)) || (rc = emit_rows(t))) return rc;
        KSP_HIP(hipEventRecord(ev[4], nullptr));
        return add_times(4);
    }

    int run(u64* n_rows, ksp_gather_stats* stats) {
        int rc = KSP_OK;
        if ((rc = setup())) return rc;
        for (u32 index = 0; index < n_tiles; ++index)
            if ((rc = run_tile(index))) return rc;
        S.rows = rows_done;
        *n_rows = rows_done;
        if (stats) *stats = S;
        if (!h_rows && rows_done > capacity) {
            ksp::set_error(std::string(who) + ": " + std::to_string(rows_done) + " rows, room for " + std::to_string(capacity));
            return KSP_E_OVERFLOW;
        }
        return KSP_OK;
    }
};

// what the two device entries do behind their own first refusals
template <class Row>
int gather_device_entry(const char* who, const int device, const u64* d_db_keys, const u64* h_db_off, const u32 n_db, const u64* d_q_keys, const u32* d_q_abund, const u64* h_q_off,
                        const u32 n_q, const u32 min_hashes, const u32 max_matches, Row* d_rows, const u64 capacity, u64* n_rows, ksp_gather_stats* stats) {
    GatherSwitches W;
    if (const int rc = check_gather_args(who, d_db_keys, h_db_off, n_db, d_q_keys, h_q_off, n_q, min_hashes, n_rows)) return rc;
    if (!d_rows && capacity) { ksp::set_error(std::string(who) + ": d_rows is NULL but capacity is not 0"); return KSP_E_ARG; }
    if (const int rc = read_switches(who, W)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    return GatherCall<Row>{who, W, d_db_keys, h_db_off, n_db, d_q_keys, d_q_abund, h_q_off, n_q, min_hashes, max_matches, d_rows, capacity, nullptr}.run(n_rows, stats);
}

// what the two host entries do behind their own first refusals; q_abund: the weighted call's, NULL for the other
template <class Row>
int gather_host_entry(const char* who, const u64* db_keys, const u64* db_off, const u32 n_db, const u64* q_keys, const u32* q_abund, const u64* q_off, const u32 n_q,
                      const u32 min_hashes, const u32 max_matches, const int device, Row** rows, u64* n_rows, ksp_gather_stats* stats) {
    GatherSwitches W;
    if (const int rc = check_gather_args(who, db_keys, db_off, n_db, q_keys, q_off, n_q, min_hashes, n_rows)) return rc;
    if (const int rc = read_switches(who, W)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    const u64 n_dbk = db_off[n_db], n_qk = q_off[n_q];
    u64 *d_db = nullptr, *d_q = nullptr, found = 0;
    u32* d_a = nullptr;
    std::vector<Row> got;
    if ((rc = q_abund ? ksp::device_fits(who, 8ull * (n_dbk + n_qk + 2) + 4ull * (n_qk + 1), "the keys of both sides and the queries' abundances")
                      : ksp::device_fits(who, 8ull * (n_dbk + n_qk + 2), "the keys of both sides")))
        return rc;
    if ((rc = query_upload_keys(A, db_keys, n_dbk, q_keys, n_qk, &d_db, &d_q))) return rc;
    if (q_abund) {
        if ((rc = A.alloc(&d_a, (size_t)n_qk + 1))) return rc;
        KSP_HIP(hipMemcpy(d_a, q_abund, (size_t)n_qk * 4, hipMemcpyHostToDevice));
    }
    try {
        rc = GatherCall<Row>{who, W, d_db, db_off, n_db, d_q, d_a, q_off, n_q, min_hashes, max_matches, nullptr, 0, &got}.run(&found, stats);
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        rc = KSP_E_LIMIT;
    }
    if (rc != KSP_OK) return rc;
    Row* const out = (Row*)std::malloc(std::max<size_t>(got.size(), 1) * sizeof(Row));
    if (!out) { ksp::set_error(std::string(who) + ": out of host memory"); return KSP_E_LIMIT; }
    if (!got.empty()) std::memcpy(out, got.data(), got.size() * sizeof(Row));
    *rows = out;
    *n_rows = found;
    return KSP_OK;
}

}  // namespace

extern "C" int ksp_gather_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys, const uint64_t* h_q_offsets,
                                 uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, ksp_gather_row* d_rows, uint64_t capacity, uint64_t* n_rows, ksp_gather_stats* stats) {
    return gather_device_entry<ksp_gather_row>("ksp_gather_device", device, d_db_keys, h_db_offsets, n_db, d_q_keys, nullptr, h_q_offsets, n_q, min_hashes, max_matches, d_rows, capacity,
                                               n_rows, stats);
}

extern "C" int ksp_gather_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint64_t* q_offsets, uint32_t n_q,
                               uint32_t min_hashes, uint32_t max_matches, int device, ksp_gather_row** rows, uint64_t* n_rows, ksp_gather_stats* stats) {
    const char* who = "ksp_gather_host";
    if (!rows) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return gather_host_entry<ksp_gather_row>(who, db_keys, db_offsets, n_db, q_keys, nullptr, q_offsets, n_q, min_hashes, max_matches, device, rows, n_rows, stats);
}

extern "C" int ksp_gather_abund_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys, const uint32_t* d_q_abund,
                                       const uint64_t* h_q_offsets, uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, ksp_gather_wrow* d_rows, uint64_t capacity,
                                       uint64_t* n_rows, ksp_gather_stats* stats) {
    const char* who = "ksp_gather_abund_device";
    if (!d_q_abund) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return gather_device_entry<ksp_gather_wrow>(who, device, d_db_keys, h_db_offsets, n_db, d_q_keys, d_q_abund, h_q_offsets, n_q, min_hashes, max_matches, d_rows, capacity, n_rows, stats);
}

extern "C" int ksp_gather_abund_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint32_t* q_abund, const uint64_t* q_offsets,
                                     uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, int device, ksp_gather_wrow** rows, uint64_t* n_rows, ksp_gather_stats* stats) {
    const char* who = "ksp_gather_abund_host";
    if (!rows || !q_abund) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return gather_host_entry<ksp_gather_wrow>(who, db_keys, db_offsets, n_db, q_keys, q_abund, q_offsets, n_q, min_hashes, max_matches, device, rows, n_rows, stats);
}
