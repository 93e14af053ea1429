// Dereplication: the greedy representatives of the containment graph and, for every other source, the
// representative that stands for it — what a user of the reference's `repr_sketches` ranking (repr.hip) goes on to compute on
// the host — from the join's edge records while they are in HBM, or from the (a, b) pairs of an existing TSV.
//
// Definition: a record is kept when its column passes the text test of `repr_sketches` (one compare against the critical float
// of ksp::repr_critical, as k_degree makes it; a NaN never passes); degree[v] counts the kept records naming v; the nodes are
// ranked by (degree descending, node ascending), ALL of them; walking the nodes in rank order, a node is a representative
// unless a kept neighbour of smaller rank is one, and otherwise a member of the smallest-ranked representative among its kept
// neighbours, through the lowest-index kept record between the two.  Self pairs count for the degree and for nothing else.
// That is the lexicographically-first maximal independent set of the kept graph in rank order: sequential as written,
// parallel in rounds.
//   rank      the counting kernel and the key kernel of repr.hip (ksp::degree_keys_on_device), one radix sort over the keys of
//             all nodes, k_derep_rank: rank[node] = position
//   pairs     k_derep_count / scan / k_derep_scatter: a STABLE compaction of the kept records that are no self pairs into
//             (lo, hi, index), lo the end of smaller rank: 12 bytes per pair for everything that follows
//   rounds    k_derep_pairs over the live pairs: state[lo] == IN knocks hi OUT, both UNDECIDED stamps blocked[hi] with the round;
//             k_derep_nodes: an UNDECIDED node without this round's stamp becomes IN.  A node turns IN only when every
//             smaller-ranked neighbour was read as decided and none as IN, so a stale read of a neighbour that is being knocked
//             OUT in the same pass delays a decision by a round and never changes it.  The smallest-ranked undecided node is
//             never stamped, so every round decides a node; the host reads one pair of counts per round and bounds the loop.
//   compact   a pair is dead once hi is decided or lo is OUT; when at most half of the list is live it is compacted
//             (k_derep_live_count / scan / k_derep_live_scatter, on a state no kernel is changing)
//   tail      at KSP_DEREP_TAIL_PAIRS live pairs or fewer ONE workgroup of 1 024 threads runs the remaining rounds with
//             __syncthreads() between the passes instead of dispatches (a path needs n / 2 rounds); KSP_DEREP_TAIL=0: never
//   assign    k_derep_assign over ALL oriented pairs with the final states: 64-bit atomicMin of (rank of the IN end, index)
//             into the OUT end — after the rounds, because a smaller-ranked representative may be decided later than the one
//             that knocked the node out; k_derep_finish: rep[] and via[]
// Every edge pass owns chunks of KSP_DEREP_CHUNK_EDGES consecutive entries per workgroup, as the containment cut does
// (cut.hip), and no workgroup ever waits on another.  The host drives and bounds every loop.
#include <cerrno>
#include <cmath>
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
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "../../include/kspider_amd.h"
#include "cluster_inputs.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "partial_file.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kDerepChunk = KSP_DEREP_CHUNK_EDGES;   // (the reasons for 2 048 entries per 256 threads: cut.hip)
constexpr int kDerepThreads = 256;
constexpr int kDerepWaves = kDerepThreads / 64;
constexpr int kDerepIters = (int)(kDerepChunk / kDerepThreads);   // entries per lane and chunk
constexpr int kTailThreads = 1024;
constexpr u32 kUndecided = 0, kIn = 1, kOut = 2;
constexpr u32 kNone = 0xFFFFFFFFu;
constexpr unsigned long long kNoBest = ~0ull;
static_assert(kDerepIters * kDerepThreads == (int)kDerepChunk, "a chunk is whole ballots of every wave");

thread_local ksp::DerepTrace g_trace;   // (ksp_debug_derep_rounds)

// first entry of wave `wave` in chunk `chunk`: wave w owns the entries [w * 512, (w + 1) * 512) of its chunk
__device__ inline u64 derep_wave_base(const u64 chunk, const u32 wave) { return chunk * kDerepChunk + (u64)wave * (kDerepIters * 64); }

__global__ void k_derep_rank(const u64* __restrict__ sorted, const u32 n, u32* __restrict__ rank) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rank[(u32)sorted[i]] = (u32)i;
}

// The ends of a chunk's entries into registers, all loads in flight before the first is used.  kRecords: the join's records
// (`shared` beside the ends); else plain (a[], b[]) pairs (the TSV form: the host applied the text test).
template <bool kRecords>
__device__ inline void derep_load(const ksp_edge* __restrict__ ed, const u32* __restrict__ a, const u32* __restrict__ b, const u64 n, const u64 base,
                                  const u32 lane, u32 (&s)[kDerepIters], u32 (&t)[kDerepIters], u64 (&sh)[kDerepIters]) {
#pragma unroll
    for (int k = 0; k < kDerepIters; ++k) {
        const u64 e = base + (u64)k * 64 + lane;
        s[k] = t[k] = kNone;
        sh[k] = 0;
        if (e < n) {
            if (kRecords) {
                const ksp_edge x = ed[e];
                s[k] = x.source_1; t[k] = x.source_2; sh[k] = x.shared;
            } else {
                s[k] = a[e]; t[k] = b[e];
            }
        }
    }
}
// An entry becomes an oriented pair when both ends are nodes, it is no self pair and (kRecords) its column passes the text test:
// !(v < vcrit) && v == v, exactly as k_degree counts it.  (An end of kNone, an entry behind the list, is never below n_nodes.)
template <bool kRecords>
__device__ inline bool derep_kept(const u32 s, const u32 t, const u64 sh, const u32 n_nodes, const u32* __restrict__ cnt, const int col, const float vcrit) {
    if (s >= n_nodes || t >= n_nodes || s == t) return false;
    if (!kRecords) return true;
    const float v = edge_col_value(ksp_edge{s, t, sh}, cnt, col);
    return !(v < vcrit) && v == v;
}

template <bool kRecords>
__global__ __launch_bounds__(kDerepThreads) void k_derep_count(const ksp_edge* __restrict__ ed, const u32* __restrict__ a, const u32* __restrict__ b, const u64 n,
                                                               const u64 n_chunks, const u32 n_nodes, const u32* __restrict__ cnt, const int col,
                                                               const float vcrit, u64* __restrict__ chunk_count) {
    __shared__ u32 wave_kept[kDerepWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        u32 s[kDerepIters], t[kDerepIters];
        u64 sh[kDerepIters];
        derep_load<kRecords>(ed, a, b, n, derep_wave_base(chunk, wave), lane, s, t, sh);
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) kept += (u32)__popcll(__ballot(derep_kept<kRecords>(s[k], t[k], sh[k], n_nodes, cnt, col, vcrit)));
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 sum = 0;
            for (int w = 0; w < kDerepWaves; ++w) sum += wave_kept[w];
            chunk_count[chunk] = sum;
        }
        __syncthreads();   // (wave_kept is written again for the next chunk)
    }
}

// The same chunks again: pair p of the kept entries, in their input order, is (lo, hi, index) with lo the end of smaller rank.
template <bool kRecords>
__global__ __launch_bounds__(kDerepThreads) void k_derep_scatter(const ksp_edge* __restrict__ ed, const u32* __restrict__ a, const u32* __restrict__ b, const u64 n,
                                                                 const u64 n_chunks, const u32 n_nodes, const u32* __restrict__ cnt, const int col,
                                                                 const float vcrit, const u64* __restrict__ chunk_off, const u32* __restrict__ rank,
                                                                 u32* __restrict__ lo, u32* __restrict__ hi, u32* __restrict__ index) {
    __shared__ u32 wave_kept[kDerepWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;   // the lanes before mine
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = derep_wave_base(chunk, wave);
        u32 s[kDerepIters], t[kDerepIters];
        u64 sh[kDerepIters];
        unsigned long long bal[kDerepIters];
        derep_load<kRecords>(ed, a, b, n, base, lane, s, t, sh);
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            bal[k] = __ballot(derep_kept<kRecords>(s[k], t[k], sh[k], n_nodes, cnt, col, vcrit));
            kept += (u32)__popcll(bal[k]);
        }
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        u64 pos = chunk_off[chunk];
        for (u32 w = 0; w < wave; ++w) pos += wave_kept[w];
        __syncthreads();   // (wave_kept is written again for the next chunk)
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            if ((bal[k] >> lane) & 1) {
                const u64 p = pos + (u64)__popcll(bal[k] & below);
                const bool first = rank[s[k]] < rank[t[k]];
                lo[p] = first ? s[k] : t[k];
                hi[p] = first ? t[k] : s[k];
                index[p] = (u32)(base + (u64)k * 64 + lane);   // (below 2^32 - 1: larger lists are refused)
            }
            pos += (u64)__popcll(bal[k]);
        }
    }
}

__global__ void k_derep_init(u32* __restrict__ state, u32* __restrict__ blocked, unsigned long long* __restrict__ best, const u32 n) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v < n) { state[v] = kUndecided; blocked[v] = 0; best[v] = kNoBest; }
}

// What one pair does in a round.  state[] is read while other lanes of the same pass write it (only ever UNDECIDED -> OUT here):
// every outcome of such a read is allowed for (the head of this file).  Returns whether the pair was read as live.
__device__ inline bool derep_pair_step(const u32 l, const u32 h, u32* state, u32* blocked, const u32 round) {
    if (state[h] != kUndecided) return false;
    const u32 sl = state[l];
    if (sl == kIn) { state[h] = kOut; return false; }
    if (sl == kUndecided) { blocked[h] = round; return true; }
    return false;
}

// One pass over the live pairs.  *live += the pairs read with both ends UNDECIDED: every other pair is dead for good.
__global__ __launch_bounds__(kDerepThreads) void k_derep_pairs(const u32* __restrict__ lo, const u32* __restrict__ hi, const u64 n, const u64 n_chunks,
                                                               u32* state, u32* blocked, const u32 round, unsigned long long* live) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = derep_wave_base(chunk, wave);
        u32 l[kDerepIters], h[kDerepIters];
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            const u64 p = base + (u64)k * 64 + lane;
            l[k] = h[k] = 0;
            if (p < n) { l[k] = lo[p]; h[k] = hi[p]; }
        }
        u32 alive = 0;
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            const u64 p = base + (u64)k * 64 + lane;
            alive += (u32)__popcll(__ballot(p < n && derep_pair_step(l[k], h[k], state, blocked, round)));
        }
        if (lane == 0 && alive) atomicAdd(live, (unsigned long long)alive);
    }
}

// An UNDECIDED node that no pair stamped in this round has no undecided and no IN neighbour of smaller rank: IN.
// *undecided += the nodes that stay UNDECIDED.
__global__ void k_derep_nodes(u32* __restrict__ state, const u32* __restrict__ blocked, const u32 n, const u32 round, u32* __restrict__ undecided) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool waits = false;
    if (v < n && state[v] == kUndecided) {
        if (blocked[v] != round) state[v] = kIn;
        else waits = true;
    }
    const unsigned long long b = __ballot(waits);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(undecided, (u32)__popcll(b));
}

// A pair stays in the list while hi is UNDECIDED and lo is not OUT.  Both passes of a compaction run on a state no kernel is
// changing, so the counts and the positions agree.
__device__ inline bool derep_live(const u32 l, const u32 h, const u32* __restrict__ state) { return state[h] == kUndecided && state[l] != kOut; }

__global__ __launch_bounds__(kDerepThreads) void k_derep_live_count(const u32* __restrict__ lo, const u32* __restrict__ hi, const u64 n, const u64 n_chunks,
                                                                    const u32* __restrict__ state, u64* __restrict__ chunk_count) {
    __shared__ u32 wave_kept[kDerepWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = derep_wave_base(chunk, wave);
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            const u64 p = base + (u64)k * 64 + lane;
            kept += (u32)__popcll(__ballot(p < n && derep_live(lo[p], hi[p], state)));
        }
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 sum = 0;
            for (int w = 0; w < kDerepWaves; ++w) sum += wave_kept[w];
            chunk_count[chunk] = sum;
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(kDerepThreads) void k_derep_live_scatter(const u32* __restrict__ lo, const u32* __restrict__ hi, const u64 n, const u64 n_chunks,
                                                                      const u32* __restrict__ state, const u64* __restrict__ chunk_off,
                                                                      u32* __restrict__ out_lo, u32* __restrict__ out_hi) {
    __shared__ u32 wave_kept[kDerepWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = derep_wave_base(chunk, wave);
        u32 l[kDerepIters], h[kDerepIters];
        unsigned long long bal[kDerepIters];
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            const u64 p = base + (u64)k * 64 + lane;
            l[k] = h[k] = 0;
            if (p < n) { l[k] = lo[p]; h[k] = hi[p]; }
            bal[k] = __ballot(p < n && derep_live(l[k], h[k], state));
            kept += (u32)__popcll(bal[k]);
        }
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        u64 pos = chunk_off[chunk];
        for (u32 w = 0; w < wave; ++w) pos += wave_kept[w];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            if ((bal[k] >> lane) & 1) {
                const u64 p = pos + (u64)__popcll(bal[k] & below);
                out_lo[p] = l[k];
                out_hi[p] = h[k];
            }
            pos += (u64)__popcll(bal[k]);
        }
    }
}

// the UNDECIDED nodes, in any order, for the tail: one append per wave
__global__ void k_derep_waiting(const u32* __restrict__ state, const u32 n, u32* __restrict__ list, u32* __restrict__ count) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 lane = threadIdx.x & 63;
    const bool waits = v < n && state[v] == kUndecided;
    const unsigned long long b = __ballot(waits);
    u32 base = 0;
    if (lane == 0 && b) base = atomicAdd(count, (u32)__popcll(b));
    base = (u32)__shfl((int)base, 0);
    if (waits) list[base + (u32)__popcll(b & ((1ull << lane) - 1))] = (u32)v;
}

// The remaining rounds by ONE workgroup: the same two passes — over the n_live live pairs, then over the n_waiting nodes that
// were UNDECIDED when it started — separated by __syncthreads() and not by dispatches.  A round decides at least one node, so
// n_waiting rounds suffice and one more would find nothing: the loop is bounded by n_waiting + 1 and ends when a count over
// the workgroup finds no UNDECIDED node.  out[0] = the rounds that ran, out[1] = the nodes still UNDECIDED (0 unless the bound
// was hit, which the host reports).  Rounds are stamped round0 + 1, round0 + 2, ...
__global__ __launch_bounds__(kTailThreads) void k_derep_tail(const u32* __restrict__ lo, const u32* __restrict__ hi, const u32 n_live,
                                                             const u32* __restrict__ waiting, const u32 n_waiting, u32* state, u32* blocked,
                                                             const u32 round0, u32* __restrict__ out) {
    __shared__ u32 s_left;
    u32 left = n_waiting, rounds = 0;
    for (u64 it = 0; it < (u64)n_waiting + 1 && left; ++it) {
        const u32 round = round0 + 1 + (u32)it;
        if (threadIdx.x == 0) s_left = 0;
        for (u32 p = threadIdx.x; p < n_live; p += kTailThreads) derep_pair_step(lo[p], hi[p], state, blocked, round);
        __syncthreads();   // every stamp and every OUT of this round is made (and s_left is 0)
        u32 mine = 0;
        for (u32 j = threadIdx.x; j < n_waiting; j += kTailThreads) {
            const u32 v = waiting[j];
            if (state[v] != kUndecided) continue;
            if (blocked[v] != round) state[v] = kIn;
            else ++mine;
        }
        if (mine) atomicAdd(&s_left, mine);
        __syncthreads();   // every IN of this round is made, s_left is complete
        left = s_left;
        ++rounds;
        __syncthreads();   // (s_left is reset by thread 0 for the next round)
    }
    if (threadIdx.x == 0) { out[0] = rounds; out[1] = left; }
}

// Every oriented pair with one IN and one OUT end offers (rank of the IN end, index) to the OUT end: the smallest word wins —
// the smallest-ranked representative, and among its records the lowest index.
__global__ __launch_bounds__(kDerepThreads) void k_derep_assign(const u32* __restrict__ lo, const u32* __restrict__ hi, const u32* __restrict__ index,
                                                                const u64 n, const u64 n_chunks, const u32* __restrict__ state,
                                                                const u32* __restrict__ rank, unsigned long long* best) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = derep_wave_base(chunk, wave);
#pragma unroll
        for (int k = 0; k < kDerepIters; ++k) {
            const u64 p = base + (u64)k * 64 + lane;
            if (p >= n) continue;
            const u32 l = lo[p], h = hi[p];
            const u32 sl = state[l], sh = state[h];
            if (sl == kIn && sh == kOut) atomicMin(&best[h], ((unsigned long long)rank[l] << 32) | index[p]);
            else if (sl == kOut && sh == kIn) atomicMin(&best[l], ((unsigned long long)rank[h] << 32) | index[p]);
        }
    }
}

// rep[v] / via[v]; a node that is neither IN nor an OUT with an offer gets kNone in rep[] (the host reports it)
__global__ void k_derep_finish(const u32* __restrict__ state, const unsigned long long* __restrict__ best, const u64* __restrict__ sorted, const u32 n,
                               u32* __restrict__ rep, u32* __restrict__ via) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const u32 st = state[v];
    const unsigned long long w = best[v];
    u32 r = kNone, e = kNone;
    if (st == kIn) r = (u32)v;
    else if (st == kOut && w != kNoBest && (w >> 32) < n) { r = (u32)sorted[w >> 32]; e = (u32)w; }
    rep[v] = r;
    via[v] = e;
}

// what one call holds on the device (memory of the call's DeviceArena)
struct DerepBufs {
    // per node (52 bytes)
    u32 *degree = nullptr, *rank = nullptr, *state = nullptr, *blocked = nullptr, *rep = nullptr, *via = nullptr, *waiting = nullptr;
    u64 *keys = nullptr, *sorted = nullptr;
    unsigned long long* best = nullptr;
    // per chunk of the entries (16 bytes): the counts and their exclusive scan, used again by every compaction
    u64 *chunk_count = nullptr, *chunk_off = nullptr;
    // per oriented pair (12 bytes) and the two lists the compactions alternate between (half the pairs each: 8 bytes per pair)
    u32 *lo = nullptr, *hi = nullptr, *index = nullptr, *live_lo[2] = {nullptr, nullptr}, *live_hi[2] = {nullptr, nullptr};
    unsigned long long* counts = nullptr;   // [0] live pairs of a pass, [1] (as u32) undecided nodes / waiting nodes, [2] (as 2 x u32) the tail's out[]
    void* tmp = nullptr;                    // the library's scratch: the larger of the sort's and the scan's
    size_t tmp_bytes = 0;
};

// exclusive scan of B.chunk_count[0 .. n_chunks] (the entry behind the last chunk is 0) into B.chunk_off; *total = the sum
int derep_scan(DerepBufs& B, const u64 n_chunks, u64* total) {
    int rc = KSP_OK;
    size_t tb = B.tmp_bytes;
    KSP_TRY_HIP(hipMemsetAsync(B.chunk_count + n_chunks, 0, 8, nullptr));
    KSP_TRY_HIP(rocprim::exclusive_scan(B.tmp, tb, B.chunk_count, B.chunk_off, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    KSP_TRY_HIP(hipMemcpy(total, B.chunk_off + n_chunks, 8, hipMemcpyDeviceToHost));
done:
    return rc;
}

// The selection on the CURRENT device over n_edges > 0 entries — records cut by vcrit (d_edges) or (d_a, d_b) pairs — and
// n_nodes > 0 nodes.  Nothing is written to the caller before everything has succeeded.
int derep_on_device(const u32 N, const ksp_edge* d_edges, const u32* d_a, const u32* d_b, const u64 n, const u32* d_cnt, const int col, const float vcrit,
                    u32* h_rep, u32* h_via, u32* h_rank, u32* h_degree, u32* n_reps, ksp::DerepTrace& T) {
    int rc = KSP_OK;
    DerepBufs B;
    ksp::DeviceArena A;
    ksp::WorkgroupCap G;   // of the edge passes: one workgroup per chunk up to 8 per CU, the rest by the chunk loop
    const u64 n_chunks = (n + kDerepChunk - 1) / kDerepChunk;
    const unsigned gn = (unsigned)(((u64)N + 255) / 256);
    const char* tail_env = std::getenv("KSP_DEREP_TAIL");   // "0": host-driven rounds to the end (tests)
    const bool use_tail = !(tail_env && std::strcmp(tail_env, "0") == 0);
    size_t tb_sort = 0, tb_scan = 0;
    u64 n_pairs = 0;
    std::vector<u32> rep, via;
    if ((rc = ksp::workgroup_cap("KSP_DEREP_MAX_WORKGROUPS", "dereplicate", G))) return rc;
    // ---- the arrays per node and per chunk, and the library's scratch: sized and checked first
    KSP_TRY_HIP(rocprim::radix_sort_keys(nullptr, tb_sort, (u64*)nullptr, (u64*)nullptr, (size_t)N, 0, 64, (hipStream_t) nullptr));
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, (u64*)nullptr, (u64*)nullptr, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    B.tmp_bytes = std::max<size_t>(std::max(tb_sort, tb_scan), 8);
    if ((rc = ksp::device_fits("dereplicate", 52ull * N + 16ull * (n_chunks + 1) + B.tmp_bytes + 32, "52 per node, 16 per 2 048 records, the sort's scratch"))) return rc;
    for (u32** p : {&B.degree, &B.rank, &B.state, &B.blocked, &B.rep, &B.via, &B.waiting})
        if ((rc = A.alloc(p, (size_t)N))) return rc;
    if ((rc = A.alloc(&B.keys, (size_t)N)) || (rc = A.alloc(&B.sorted, (size_t)N)) || (rc = A.alloc(&B.best, (size_t)N))) return rc;
    if ((rc = A.alloc(&B.chunk_count, (size_t)(n_chunks + 1))) || (rc = A.alloc(&B.chunk_off, (size_t)(n_chunks + 1)))) return rc;
    if ((rc = A.alloc(&B.counts, 4)) || (rc = A.alloc_bytes(&B.tmp, B.tmp_bytes))) return rc;
    // ---- degrees and the rank of every node
    if ((rc = ksp::degree_keys_on_device(N, d_edges, d_a, d_b, n, d_cnt, col, vcrit, B.degree, B.keys))) return rc;
    {
        size_t tb = B.tmp_bytes;
        KSP_TRY_HIP(rocprim::radix_sort_keys(B.tmp, tb, B.keys, B.sorted, (size_t)N, 0, 64, (hipStream_t) nullptr));
    }
    hipLaunchKernelGGL(k_derep_rank, dim3(gn), dim3(256), 0, nullptr, (const u64*)B.sorted, N, B.rank);
    hipLaunchKernelGGL(k_derep_init, dim3(gn), dim3(256), 0, nullptr, B.state, B.blocked, B.best, N);
    KSP_TRY_HIP(hipGetLastError());
    // ---- the oriented kept pairs
    if (d_edges) hipLaunchKernelGGL(k_derep_count<true>, dim3(G.grid_of(n_chunks)), dim3(kDerepThreads), 0, nullptr, d_edges, d_a, d_b, n, n_chunks, N, d_cnt, col, vcrit, B.chunk_count);
    else hipLaunchKernelGGL(k_derep_count<false>, dim3(G.grid_of(n_chunks)), dim3(kDerepThreads), 0, nullptr, d_edges, d_a, d_b, n, n_chunks, N, d_cnt, col, vcrit, B.chunk_count);
    KSP_TRY_HIP(hipGetLastError());
    if ((rc = derep_scan(B, n_chunks, &n_pairs))) return rc;
    if (n_pairs > n) { ksp::set_error("dereplicate: more kept pairs than records"); return KSP_E_HIP; }
    T.kept = n_pairs;
    if (n_pairs) {
        const u64 half = n_pairs / 2;
        if ((rc = ksp::device_fits("dereplicate", 12ull * n_pairs + 16ull * half, "12 per kept pair, 8 more for the live lists"))) return rc;
        for (u32** p : {&B.lo, &B.hi, &B.index})
            if ((rc = A.alloc(p, (size_t)n_pairs))) return rc;
        if (half)
            for (int i = 0; i < 2; ++i)
                if ((rc = A.alloc(&B.live_lo[i], (size_t)half)) || (rc = A.alloc(&B.live_hi[i], (size_t)half))) return rc;
        if (d_edges) hipLaunchKernelGGL(k_derep_scatter<true>, dim3(G.grid_of(n_chunks)), dim3(kDerepThreads), 0, nullptr, d_edges, d_a, d_b, n, n_chunks, N, d_cnt, col, vcrit, (const u64*)B.chunk_off, (const u32*)B.rank, B.lo, B.hi, B.index);
        else hipLaunchKernelGGL(k_derep_scatter<false>, dim3(G.grid_of(n_chunks)), dim3(kDerepThreads), 0, nullptr, d_edges, d_a, d_b, n, n_chunks, N, d_cnt, col, vcrit, (const u64*)B.chunk_off, (const u32*)B.rank, B.lo, B.hi, B.index);
        KSP_TRY_HIP(hipGetLastError());
    }
    // ---- the rounds
    {
        const u32 *cur_lo = B.lo, *cur_hi = B.hi;   // the list of the passes: all pairs, then what the compactions left
        u64 len = n_pairs;
        int next_buf = 0;
        u32* const d_undecided = (u32*)(B.counts + 1);
        u32* const d_tail_out = (u32*)(B.counts + 2);
        // stable compaction of the list into the other live buffer: the pairs whose hi is UNDECIDED and whose lo is not OUT
        auto compact = [&]() -> int {
            int rc = KSP_OK;
            const u64 chunks = (len + kDerepChunk - 1) / kDerepChunk;
            u64 kept = 0;
            hipLaunchKernelGGL(k_derep_live_count, dim3(G.grid_of(chunks)), dim3(kDerepThreads), 0, nullptr, cur_lo, cur_hi, len, chunks, (const u32*)B.state, B.chunk_count);
            KSP_TRY_HIP(hipGetLastError());
            if ((rc = derep_scan(B, chunks, &kept))) return rc;
            if (kept > n_pairs / 2) { ksp::set_error("dereplicate: a compaction kept more pairs than its list holds"); return KSP_E_HIP; }
            if (kept)
                hipLaunchKernelGGL(k_derep_live_scatter, dim3(G.grid_of(chunks)), dim3(kDerepThreads), 0, nullptr, cur_lo, cur_hi, len, chunks, (const u32*)B.state,
                                   (const u64*)B.chunk_off, B.live_lo[next_buf], B.live_hi[next_buf]);
            KSP_TRY_HIP(hipGetLastError());
            cur_lo = B.live_lo[next_buf];
            cur_hi = B.live_hi[next_buf];
            next_buf ^= 1;
            len = kept;
        done:
            return rc;
        };
        const u64 max_rounds = (u64)N + 1;   // every round decides a node; one more would find nothing to do
        u64 round = 0;
        while (true) {
            if (++round > max_rounds) { ksp::set_error("dereplicate: more than " + std::to_string(max_rounds) + " rounds"); return KSP_E_HIP; }
            unsigned long long h_counts[2] = {0, 0};
            const u64 chunks = (len + kDerepChunk - 1) / kDerepChunk;
            KSP_TRY_HIP(hipMemsetAsync(B.counts, 0, 16, nullptr));
            if (len) hipLaunchKernelGGL(k_derep_pairs, dim3(G.grid_of(chunks)), dim3(kDerepThreads), 0, nullptr, cur_lo, cur_hi, len, chunks, B.state, B.blocked, (u32)round, B.counts);
            hipLaunchKernelGGL(k_derep_nodes, dim3(gn), dim3(256), 0, nullptr, B.state, (const u32*)B.blocked, N, (u32)round, d_undecided);
            KSP_TRY_HIP(hipGetLastError());
            KSP_TRY_HIP(hipMemcpy(h_counts, B.counts, 16, hipMemcpyDeviceToHost));
            ++T.dispatched;
            const u64 live = h_counts[0];
            const u32 undecided = (u32)h_counts[1];
            if (undecided == 0) break;
            if (live > len) { ksp::set_error("dereplicate: more live pairs than the list holds"); return KSP_E_HIP; }
            // Compaction rule: when at most half of the list is live.  Every compaction then at least halves the list, so all of
            // them together read and write less than twice the first list, and the two live buffers of n_pairs / 2 always fit
            // (the pairs a compaction keeps are among those the pass before it read as live).
            if (live <= len / 2 && (rc = compact())) return rc;
            if (use_tail && live <= KSP_DEREP_TAIL_PAIRS) {   // (the list is then shorter than twice that)
                u32 h_out[2] = {0, 0}, waiting = 0;
                KSP_TRY_HIP(hipMemsetAsync(d_undecided, 0, 4, nullptr));
                hipLaunchKernelGGL(k_derep_waiting, dim3(gn), dim3(256), 0, nullptr, (const u32*)B.state, N, B.waiting, d_undecided);
                KSP_TRY_HIP(hipGetLastError());
                KSP_TRY_HIP(hipMemcpy(&waiting, d_undecided, 4, hipMemcpyDeviceToHost));
                if (waiting != undecided) { ksp::set_error("dereplicate: the tail's node list does not match the count of the round before"); return KSP_E_HIP; }
                T.live_at_tail = live;   // (the list it is handed may still hold dead pairs: fewer than as many again)
                hipLaunchKernelGGL(k_derep_tail, dim3(1), dim3(kTailThreads), 0, nullptr, cur_lo, cur_hi, (u32)len, (const u32*)B.waiting, waiting, B.state, B.blocked,
                                   (u32)round, d_tail_out);
                KSP_TRY_HIP(hipGetLastError());
                KSP_TRY_HIP(hipMemcpy(h_out, d_tail_out, 8, hipMemcpyDeviceToHost));
                T.tail = h_out[0];
                if (h_out[1]) { ksp::set_error("dereplicate: the tail left " + std::to_string(h_out[1]) + " nodes undecided after " + std::to_string(h_out[0]) + " rounds"); return KSP_E_HIP; }
                break;
            }
        }
    }
    // ---- the assignment, with the final states, over ALL oriented pairs
    if (n_pairs) {
        const u64 chunks = (n_pairs + kDerepChunk - 1) / kDerepChunk;
        hipLaunchKernelGGL(k_derep_assign, dim3(G.grid_of(chunks)), dim3(kDerepThreads), 0, nullptr, (const u32*)B.lo, (const u32*)B.hi, (const u32*)B.index, n_pairs, chunks,
                           (const u32*)B.state, (const u32*)B.rank, B.best);
    }
    hipLaunchKernelGGL(k_derep_finish, dim3(gn), dim3(256), 0, nullptr, (const u32*)B.state, (const unsigned long long*)B.best, (const u64*)B.sorted, N, B.rep, B.via);
    KSP_TRY_HIP(hipGetLastError());
    rep.resize(N);
    via.resize(N);
    KSP_TRY_HIP(hipMemcpy(rep.data(), B.rep, (size_t)N * 4, hipMemcpyDeviceToHost));
    KSP_TRY_HIP(hipMemcpy(via.data(), B.via, (size_t)N * 4, hipMemcpyDeviceToHost));
    {
        u32 reps = 0;
        for (u32 v = 0; v < N; ++v) {
            if (rep[v] == kNone || rep[v] >= N || (via[v] != kNone && via[v] >= n)) { ksp::set_error("dereplicate: node " + std::to_string(v) + " was left without a representative"); return KSP_E_HIP; }
            reps += rep[v] == v;
        }
        if (h_rank) KSP_TRY_HIP(hipMemcpy(h_rank, B.rank, (size_t)N * 4, hipMemcpyDeviceToHost));
        if (h_degree) KSP_TRY_HIP(hipMemcpy(h_degree, B.degree, (size_t)N * 4, hipMemcpyDeviceToHost));
        std::memcpy(h_rep, rep.data(), (size_t)N * 4);
        if (h_via) std::memcpy(h_via, via.data(), (size_t)N * 4);
        *n_reps = reps;
    }
done:
    return rc;
}

// nothing is kept: every node is its own representative, ranked in node order
void derep_identity(const u32 N, u32* h_rep, u32* h_via, u32* h_rank, u32* h_degree, u32* n_reps) {
    for (u32 v = 0; v < N; ++v) {
        h_rep[v] = v;
        if (h_via) h_via[v] = kNone;
        if (h_rank) h_rank[v] = v;
        if (h_degree) h_degree[v] = 0;
    }
    *n_reps = N;
}

int check_threshold(const char* who, const double threshold) {
    if (threshold != threshold) { ksp::set_error(std::string(who) + ": the threshold is NaN"); return KSP_E_ARG; }
    if (threshold < 0) { ksp::set_error(std::string(who) + ": the threshold is negative (a row without shared k-mers would pass)"); return KSP_E_ARG; }
    return KSP_OK;
}

}  // namespace

namespace ksp {
int derep_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, const double threshold,
                          uint32_t* h_rep, uint32_t* h_via, uint32_t* h_rank, uint32_t* h_degree, uint32_t* n_reps, DerepTrace* trace) {
    float vcrit = 0;
    int none_pass = 0;
    DerepTrace T;
    int rc = KSP_OK;
    repr_critical(threshold, &vcrit, &none_pass);
    if (n_edges == 0 || n_nodes == 0 || none_pass) derep_identity(n_nodes, h_rep, h_via, h_rank, h_degree, n_reps);   // no kernel runs
    else rc = derep_on_device(n_nodes, d_edges, nullptr, nullptr, n_edges, d_cnt, col, vcrit, h_rep, h_via, h_rank, h_degree, n_reps, T);
    g_trace = T;
    if (trace) *trace = T;
    return rc;
}

// "source\trepresentative\t<dist>\tneighbours\trank" and one row per name, in the order of the names, through out_path.partial
// and a rename; on a failure nothing is left behind
void write_derep_file(const std::string& out_path, const std::string& dist, const std::vector<DerepRow>& rows, const std::vector<std::string>& name_of) {
    std::string text = "source\trepresentative\t" + dist + "\tneighbours\trank\n";
    for (size_t v = 0; v < rows.size(); ++v) {
        const DerepRow& r = rows[v];
        text += name_of[v] + "\t" + name_of[r.rep] + "\t" + (r.rep == v ? std::string("-") : r.text) + "\t" + std::to_string(r.degree) + "\t" + std::to_string(r.rank) + "\n";
    }
    write_file_atomically(out_path, text);
}
}  // namespace ksp

extern "C" int ksp_edges_dereplicate(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                     double threshold, uint32_t* h_rep, uint32_t* h_via, uint32_t* h_rank, uint32_t* h_degree, uint32_t* n_reps) {
    const char* who = "ksp_edges_dereplicate";
    if (!n_reps || (n_nodes && !h_rep) || (n_edges && (!d_edges || !d_kmer_counts))) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (threshold != threshold) { ksp::set_error(std::string(who) + ": the threshold is NaN"); return KSP_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 records or more (a record's index is half of its 64-bit key)"); return KSP_E_LIMIT; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return ksp::derep_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, threshold, h_rep, h_via, h_rank, h_degree, n_reps);
}

extern "C" int ksp_debug_derep_rounds(uint64_t out[4]) {
    if (!out) { ksp::set_error("ksp_debug_derep_rounds: NULL argument"); return KSP_E_ARG; }
    out[0] = g_trace.dispatched;
    out[1] = g_trace.tail;
    out[2] = g_trace.live_at_tail;
    out[3] = g_trace.kept;
    return KSP_OK;
}

extern "C" int kspider_dereplicate(const char* index_prefix, const char* dist_type, double threshold, const char* out_path) {
    const char* who = "kspider_dereplicate";
    if (!index_prefix) { ksp::set_error(std::string(who) + ": index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "avg_cont";
    const int col = cluster_col(dt);
    if (col < 3 || col > 5) {
        ksp::set_error(std::string(who) + ": distance '" + dt + "' is not min_cont, avg_cont or max_cont" +
                       (dt == "ani" ? " (the tool reads a containment column of the pairwise TSV; the ANI column is a separate file)" : ""));
        return KSP_E_ARG;
    }
    if (const int rc = check_threshold(who, threshold)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr;
    g_trace = ksp::DerepTrace();
    try {
        // the rows that pass the text test, on the text as it stands: strtof, as a double, strictly above the threshold
        std::vector<std::string> name_of, text;
        std::vector<u32> ea, eb;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double, const std::string& t) {
            const float v = std::strtof(t.c_str(), nullptr);   // (the reader has checked that the text is a number)
            if (!((double)v > threshold)) return;
            ksp::check_row_nodes(a, b, name_of.size());
            if (ea.size() >= 0xFFFFFFFEull) throw std::runtime_error("2^32 - 1 rows or more pass (a row's index is half of its 64-bit key)");
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            text.push_back(t);
        });
        const u32 N = (u32)name_of.size();
        const u64 M = ea.size();
        std::vector<u32> rep((size_t)N), via((size_t)N), rank((size_t)N), degree((size_t)N);
        u32 n_reps = 0;
        ksp::DerepTrace T;
        if (M && N) {
            if ((rc = ksp::set_device(who, ksp::device_from_env()))) return rc;
            if ((rc = ksp::upload_pairs(A, ea.data(), eb.data(), M, &d_a, &d_b))) return rc;
            if ((rc = derep_on_device(N, nullptr, d_a, d_b, M, nullptr, 0, 0.0f, rep.data(), via.data(), rank.data(), degree.data(), &n_reps, T))) return rc;
        } else {
            derep_identity(N, rep.data(), via.data(), rank.data(), degree.data(), &n_reps);
        }
        g_trace = T;
        std::vector<ksp::DerepRow> rows((size_t)N);
        for (u32 v = 0; v < N; ++v) {
            rows[v].rep = rep[v];
            rows[v].degree = degree[v];
            rows[v].rank = rank[v];
            if (rep[v] != v) rows[v].text = text[via[v]];
        }
        ksp::write_derep_file(out_path && *out_path ? std::string(out_path) : prefix + "_kSpider_dereplicated_" + dt + ".tsv", dt, rows, name_of);
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: dereplicated " << N << " sources: " << T.kept << " records kept, " << n_reps << " representatives, " << T.dispatched
                      << " rounds and " << T.tail << " in the tail" << std::endl;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        rc = KSP_E_LIMIT;
    } catch (const std::exception& e) {
        const std::string m = e.what();
        ksp::set_error(std::string(who) + ": " + m);
        rc = m.find("2^32") != std::string::npos ? KSP_E_LIMIT : KSP_E_IO;
    }
    return rc;
}
