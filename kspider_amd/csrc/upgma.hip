// The average-linkage hierarchy (UPGMA) of the containment graph, exact, on the sparse edge list: no N x N matrix
// and no node limit.  The definition is in include/kspider_amd.h; in short:
//   q(v) = (uint64_t)((double)v * 4294967296.0); a record takes part when both ends are < n_nodes, they differ and q > 0;
//   S(A, B) = the sum of q over the records between clusters A and B; {A, B} is a candidate when S > 0; its similarity is the
//   rational S / (|A| * |B|); candidates are ordered by similarity descending (exactly: upgma_order.h), then the smaller root,
//   then the larger root; the sequential result merges the first candidate again and again, a merge being the row
//   (lo, hi, S, |lo|, |hi|) and the merged cluster's root lo.
// PARALLEL FORM (the theorem the device rests on; proof sketch in DESIGN.md 7m): in one round every cluster picks its first
// candidate pair; every pair picked by BOTH of its ends is merged, all of them at once; the surviving pairs are contracted
// (both ends relabelled, pairs inside one cluster dropped, S summed over equal pairs).  The rows of all rounds, sorted by the
// order, are exactly the sequential rows.  PROGRESS: the globally first pair is always mutual, so a round with a candidate
// merges at least one pair and the rounds are at most n_nodes - 1; a path with monotone weights needs about 0.6 * n_nodes of
// them — the bad case, not bounded away.  SHORT RUNS: a cluster merges with at most one other per round, so after relabelling
// at most 4 pairs share a key ({A, B} x {C, D}); only the fold of the raw records can meet longer runs (repeated records).
//   prep      k_upgma_prep: value, domain flag, participation and q of every record; key = (min end) << B | (max end) with
//             B = bits of n_nodes - 1; a record that takes no part gets the all-ones key (no pair has it: lo < hi <= 2^B - 1)
//   sort      rocprim::radix_sort_pairs of (key, S) over the bits [0, 2B) — a range that starts at 0
//             (tools/rocprim_bitrange_repro.hip); the all-ones keys end up last
//   fold      k_upgma_fold twice around rocprim::exclusive_scan (count per chunk, scan, place: the pattern of cut.hip): the first
//             record of every run of equal keys sums its run and lands in the live pair list (key, S), sorted and unique
//   round     k_upgma_offer: every live pair offers itself to best[] of both roots, a compare-and-swap loop under the order,
//             behind a relaxed device-scope load (k_tree_offer<true>); it compares through the pair list and size[], both
//             read-only during the kernel, so the final best[] does not depend on scheduling.  k_upgma_merge: a pair held by
//             both ends appends its row to the log (a wave-aggregated counter; the log's order is irrelevant), sets
//             map[hi] = lo and size[lo] += size[hi].  k_upgma_relabel: new keys through map[], all-ones inside one cluster,
//             and best[] of the roots it touches back to 0.  Then sort and fold again; ONE read-back per round.
//   finish    when the live pairs are at most KSP_UPGMA_TAIL_PAIRS ($KSP_UPGMA_TAIL_PAIRS; 0: never) the pair list and size[] go
//             to the host, which finishes sequentially with the same comparison: the top of a UPGMA tree merges a handful of
//             big clusters one pair per round.  The rows are the same either way.
// Every pass owns chunks of KSP_UPGMA_CHUNK_EDGES consecutive entries per 256-thread workgroup, looped by the workgroup; no
// workgroup waits on another; the host drives and bounds every loop (n_nodes rounds; a round without a merge while pairs are
// live is KSP_E_HIP with a message, never a spin).  Every count, offset and index is 64-bit.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <fstream>
#include <iostream>
#include <numeric>
#include <string>
#include <unordered_map>
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
#include "tree_newick.h"
#include "upgma_order.h"

typedef uint32_t u32;
typedef uint64_t u64;
typedef unsigned long long ull;

namespace {

constexpr u32 kChunk = KSP_UPGMA_CHUNK_EDGES;   // (the reasons for 2 048 entries per 256 threads: cut.hip; not measured here)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kIters = (int)(kChunk / kThreads);   // entries per lane and chunk
constexpr ull kDead = ~0ull;
static_assert(kIters * kThreads == (int)kChunk, "a chunk is whole ballots of every wave");
static_assert(sizeof(ksp_upgma_row) == 24, "a log row is 24 bytes");

// the counters of one call, 8 words of device memory
enum { kcMerges = 0, kcLongestRun = 1, kcDomain = 2, kcTakingPart = 3, kcLive = 4, kcLogOverflow = 5, kcWords = 8 };

thread_local ksp::UpgmaTrace g_trace;   // (ksp_debug_upgma_counts)

// the edges of one call: the join's records (ed, cnt, col) or valued pairs (a, b, val)
struct UpgmaIn {
    const ksp_edge* ed = nullptr;
    const u32* cnt = nullptr;
    int col = 0;
    const u32 *a = nullptr, *b = nullptr;
    const float* val = nullptr;
};

// first entry of wave `wave` in chunk `chunk`: wave w owns the entries [w * 512, (w + 1) * 512) of its chunk, ballot by ballot
__device__ inline u64 wave_base(const u64 chunk, const u32 wave) { return chunk * kChunk + (u64)wave * (kIters * 64); }

__device__ inline ull pair_key(const u32 s, const u32 t, const u32 B) { return ((ull)(s < t ? s : t) << B) | (ull)(s < t ? t : s); }

// Key and q of every record.  Nothing is read through an end that is no node.  The domain: a value above 1 (+inf included) of a
// record whose ends are nodes sets the flag; the host refuses the call before anything is written to the caller.
template <bool kRecords>
__global__ __launch_bounds__(kThreads) void k_upgma_prep(const UpgmaIn in, const u64 n, const u64 n_chunks, const u32 N, const u32 B, ull* __restrict__ key,
                                                          ull* __restrict__ S, ull* __restrict__ counters) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = wave_base(chunk, wave);
        u32 part = 0;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            ull kk = kDead, q = 0;
            if (e < n) {
                u32 s, t;
                float v = 0;
                bool nodes;
                if (kRecords) {
                    const ksp_edge x = in.ed[e];
                    s = x.source_1; t = x.source_2;
                    nodes = s < N && t < N;
                    if (nodes) v = edge_col_value(x, in.cnt, in.col);
                } else {
                    s = in.a[e]; t = in.b[e];
                    nodes = s < N && t < N;
                    if (nodes) v = in.val[e];
                }
                if (nodes) {
                    if (v > 1) bad = true;   // (a NaN is not above anything)
                    else if (v > 0 && s != t) q = (ull)((double)v * 4294967296.0);
                    if (q) kk = pair_key(s, t, B);
                }
                key[e] = kk;
                S[e] = q;
            }
            part += (u32)__popcll(__ballot(q != 0));
        }
        if (__ballot(bad) && lane == 0) counters[kcDomain] = 1;
        if (lane == 0 && part) atomicAdd(&counters[kcTakingPart], (ull)part);
    }
}

__global__ void k_upgma_init(u32* __restrict__ size, u32* __restrict__ map, ull* __restrict__ best, const u32 N) {
    const u32 v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < N) { size[v] = 1; map[v] = v; best[v] = 0; }
}

// The sorted entries (key, S), n of them, folded into the pair list: entry e is a HEAD when its key is not all ones and differs
// from the key before it.  kPlace false: chunk_count[chunk] = the heads of the chunk.  kPlace true: head number p (chunk_off +
// its rank in the chunk, in order) writes (key, the sum of S over its run) to out[p]; the run may leave the chunk: followers are
// only read.  kcLive = the number of heads; with track_run, kcLongestRun = the longest run summed (atomicMax over all folds).
template <bool kPlace>
__global__ __launch_bounds__(kThreads) void k_upgma_fold(const ull* __restrict__ key, const ull* __restrict__ S, const u64 n, const u64 n_chunks,
                                                          ull* __restrict__ chunk_count, const ull* __restrict__ chunk_off, ull* __restrict__ out_key,
                                                          ull* __restrict__ out_S, ull* __restrict__ counters, const int track_run) {
    __shared__ u32 wave_heads[kWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ull below = (1ull << lane) - 1;   // the lanes before mine
    if (kPlace && blockIdx.x == 0 && threadIdx.x == 0) counters[kcLive] = chunk_off[n_chunks];
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = wave_base(chunk, wave);
        ull kk[kIters], b[kIters];
        u32 heads = 0;
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            bool head = false;
            kk[k] = kDead;
            if (e < n) {
                kk[k] = key[e];
                head = kk[k] != kDead && (e == 0 || key[e - 1] != kk[k]);
            }
            b[k] = __ballot(head);
            heads += (u32)__popcll(b[k]);
        }
        if (lane == 0) wave_heads[wave] = heads;
        __syncthreads();
        if (!kPlace) {
            if (threadIdx.x == 0) {
                ull sum = 0;
                for (int w = 0; w < kWaves; ++w) sum += wave_heads[w];
                chunk_count[chunk] = sum;
            }
        } else {
            u64 pos = chunk_off[chunk];
            for (u32 w = 0; w < wave; ++w) pos += wave_heads[w];
            u32 longest = 0;
#pragma unroll
            for (int k = 0; k < kIters; ++k) {
                if ((b[k] >> lane) & 1) {
                    const u64 e = base + (u64)k * 64 + lane;
                    ull sum = S[e];
                    u64 j = e + 1;
                    while (j < n && key[j] == kk[k]) { sum += S[j]; ++j; }
                    const u64 p = pos + (u64)__popcll(b[k] & below);
                    out_key[p] = kk[k];
                    out_S[p] = sum;
                    const u64 run = j - e;
                    longest = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (longest > (u32)run ? longest : (u32)run);
                }
                pos += (u64)__popcll(b[k]);
            }
            if (track_run) {
                for (int d = 32; d; d >>= 1) {
                    const u32 o = (u32)__shfl_xor((int)longest, d);
                    longest = o > longest ? o : longest;
                }
                if (lane == 0 && longest > 1) atomicMax(&counters[kcLongestRun], (ull)longest);
            }
        }
        __syncthreads();   // (wave_heads is written again for the next chunk)
    }
}

// pair i offers itself to root c: it replaces what best[c] holds when it comes before it in the order
__device__ inline void offer_to(ull* best, const u32 c, const u64 i, const ull* __restrict__ key, const ull* __restrict__ S, const u32* __restrict__ size,
                                const u32 B, const ull mask, const ull s_i, const ull p_i, const u32 lo, const u32 hi) {
    ull cur = __hip_atomic_load(&best[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) {
        if (cur) {
            const ull kj = key[cur - 1];
            const u32 lj = (u32)(kj >> B), hj = (u32)(kj & mask);
            if (!ksp_upgma_pair_before(s_i, p_i, lo, hi, S[cur - 1], (ull)size[lj] * size[hj], lj, hj)) return;
        }
        const ull old = atomicCAS(&best[c], cur, (ull)(i + 1));
        if (old == cur) return;
        cur = old;
    }
}

// Every live pair offers itself to both of its roots: best[c] = 1 + the index of c's first candidate pair (0: none).
__global__ __launch_bounds__(kThreads) void k_upgma_offer(const ull* __restrict__ key, const ull* __restrict__ S, const u64 m, const u64 n_chunks,
                                                           const u32* __restrict__ size, const u32 B, ull* best) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ull mask = (1ull << B) - 1;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = wave_base(chunk, wave);
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const u64 i = base + (u64)k * 64 + lane;
            if (i >= m) continue;
            const ull kk = key[i], s = S[i];
            const u32 lo = (u32)(kk >> B), hi = (u32)(kk & mask);
            const ull p = (ull)size[lo] * size[hi];
            offer_to(best, lo, i, key, S, size, B, mask, s, p, lo, hi);
            offer_to(best, hi, i, key, S, size, B, mask, s, p, lo, hi);
        }
    }
}

// One thread per live pair.  A pair held by both of its ends is merged.  A cluster holds one pair, so the merged pairs of a round
// share no end: no thread reads a size or a map entry another thread of this kernel writes.
__global__ __launch_bounds__(kThreads) void k_upgma_merge(const ull* __restrict__ key, const ull* __restrict__ S, const u64 m, const u64 n_chunks,
                                                           const ull* __restrict__ best, const u32 B, u32* size, u32* __restrict__ map,
                                                           ksp_upgma_row* __restrict__ log, const u64 log_rows, ull* __restrict__ counters) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ull mask = (1ull << B) - 1, below = (1ull << lane) - 1;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = wave_base(chunk, wave);
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const u64 i = base + (u64)k * 64 + lane;
            ull kk = 0;
            u32 lo = 0, hi = 0;
            bool mutual = false;
            if (i < m) {
                kk = key[i];
                lo = (u32)(kk >> B); hi = (u32)(kk & mask);
                mutual = best[lo] == i + 1 && best[hi] == i + 1;
            }
            const ull b = __ballot(mutual);
            if (!b) continue;
            ull slot = 0;
            if (lane == (u32)(__ffsll((long long)b) - 1)) slot = atomicAdd(&counters[kcMerges], (ull)__popcll(b));
            slot = (ull)__shfl((int)(u32)slot, __ffsll((long long)b) - 1) | ((ull)(u32)__shfl((int)(u32)(slot >> 32), __ffsll((long long)b) - 1) << 32);
            if (!mutual) continue;
            slot += (ull)__popcll(b & below);
            const u32 slo = size[lo], shi = size[hi];
            if (slot < log_rows) log[slot] = ksp_upgma_row{lo, hi, S[i], slo, shi};
            else counters[kcLogOverflow] = 1;
            map[hi] = lo;
            size[lo] = slo + shi;
        }
    }
}

// Per live pair: its key under the new roots, all ones when both ends now share one; best[] of its old roots back to "none"
// (every root that held an offer is an end of a live pair, and so is every new root).
__global__ __launch_bounds__(kThreads) void k_upgma_relabel(ull* __restrict__ key, const u64 m, const u64 n_chunks, const u32* __restrict__ map, const u32 B,
                                                             ull* __restrict__ best) {
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const ull mask = (1ull << B) - 1;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = wave_base(chunk, wave);
#pragma unroll
        for (int k = 0; k < kIters; ++k) {
            const u64 i = base + (u64)k * 64 + lane;
            if (i >= m) continue;
            const ull kk = key[i];
            const u32 lo = (u32)(kk >> B), hi = (u32)(kk & mask);
            const u32 a = map[lo], b = map[hi];
            best[lo] = 0;
            best[hi] = 0;
            key[i] = a == b ? kDead : pair_key(a, b, B);
        }
    }
}

u64 chunks_of(const u64 n) { return (n + kChunk - 1) / kChunk; }

// live pairs at or below which the host finishes: KSP_UPGMA_TAIL_PAIRS, or $KSP_UPGMA_TAIL_PAIRS (0: the device to the end)
u64 tail_pairs() {
    const char* t = std::getenv("KSP_UPGMA_TAIL_PAIRS");
    if (!t || !*t) return KSP_UPGMA_TAIL_PAIRS;
    const long long v = std::atoll(t);
    return v < 0 ? 0 : (u64)v;
}

struct UpgmaBufs {
    ull *key_a = nullptr, *s_a = nullptr, *key_b = nullptr, *s_b = nullptr;   // two (key, S) buffers: the sort goes a -> b, the fold b -> a
    ull *chunk_count = nullptr, *chunk_off = nullptr;                          // per chunk and one more
    u32 *size = nullptr, *map = nullptr;
    ull* best = nullptr;
    ksp_upgma_row* log = nullptr;
    ull* counters = nullptr;
    void* tmp = nullptr;
    size_t tmp_bytes = 0;
};

// the scratch rocPRIM wants for the sort of n entries over `bits` bits and for the scan of n_chunks + 1 counts
int scratch_bytes(const u64 n, const u32 bits, size_t* out) {
    int rc = KSP_OK;
    size_t tb_sort = 0, tb_scan = 0;
    KSP_TRY_HIP(rocprim::radix_sort_pairs(nullptr, tb_sort, (ull*)nullptr, (ull*)nullptr, (ull*)nullptr, (ull*)nullptr, (size_t)n, 0u, bits, (hipStream_t) nullptr));
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, (ull*)nullptr, (ull*)nullptr, (ull)0, (size_t)(chunks_of(n) + 1), rocprim::plus<ull>(), (hipStream_t) nullptr));
    *out = std::max<size_t>(std::max(tb_sort, tb_scan), 8);
done:
    return rc;
}

// sort the first n entries of buffer a into b, fold b into a: a = the live pair list, kcLive its length
int sort_and_fold(UpgmaBufs& Bf, ksp::DeviceArena& A, const ksp::WorkgroupCap& G, const u64 n, const u32 B, const bool track_run) {
    int rc = KSP_OK;
    const u64 n_chunks = chunks_of(n);
    const unsigned grid = G.grid_of(n_chunks);
    size_t need = 0, tb = 0;
    if ((rc = scratch_bytes(n, 2 * B, &need))) return rc;
    if (need > Bf.tmp_bytes) {   // (rocPRIM asks for more at a smaller size than at the first one: not seen, but not promised either)
        if ((rc = A.alloc_bytes(&Bf.tmp, need))) return rc;
        Bf.tmp_bytes = need;
    }
    tb = Bf.tmp_bytes;
    KSP_TRY_HIP(rocprim::radix_sort_pairs(Bf.tmp, tb, Bf.key_a, Bf.key_b, Bf.s_a, Bf.s_b, (size_t)n, 0u, 2 * B, (hipStream_t) nullptr));
    KSP_TRY_HIP(hipMemsetAsync(Bf.chunk_count + n_chunks, 0, 8, nullptr));   // (the scan's last output is then the total)
    hipLaunchKernelGGL(k_upgma_fold<false>, dim3(grid), dim3(kThreads), 0, nullptr, (const ull*)Bf.key_b, (const ull*)Bf.s_b, n, n_chunks, Bf.chunk_count,
                       (const ull*)nullptr, (ull*)nullptr, (ull*)nullptr, Bf.counters, 0);
    KSP_TRY_HIP(hipGetLastError());
    tb = Bf.tmp_bytes;
    KSP_TRY_HIP(rocprim::exclusive_scan(Bf.tmp, tb, Bf.chunk_count, Bf.chunk_off, (ull)0, (size_t)(n_chunks + 1), rocprim::plus<ull>(), (hipStream_t) nullptr));
    hipLaunchKernelGGL(k_upgma_fold<true>, dim3(grid), dim3(kThreads), 0, nullptr, (const ull*)Bf.key_b, (const ull*)Bf.s_b, n, n_chunks, (ull*)nullptr,
                       (const ull*)Bf.chunk_off, Bf.key_a, Bf.s_a, Bf.counters, track_run ? 1 : 0);
    KSP_TRY_HIP(hipGetLastError());
done:
    return rc;
}

bool row_before(const ksp_upgma_row& x, const ksp_upgma_row& y) {
    return ksp_upgma_pair_before(x.sum_q, (u64)x.size_lo * x.size_hi, x.lo, x.hi, y.sum_q, (u64)y.size_lo * y.size_hi, y.lo, y.hi);
}

// The sequential definition over the live pair list (key, S) and the sizes of all nodes: the rows in merge order behind `rows`.
// O(pairs) per merge: the list is short by the time it gets here.
void host_finish(const std::vector<ull>& key, const std::vector<ull>& S, std::vector<u32>& size, const u32 B, std::vector<ksp_upgma_row>& rows) {
    const ull mask = (1ull << B) - 1;
    std::unordered_map<ull, ull> pairs;
    for (size_t i = 0; i < key.size(); ++i) pairs[key[i]] = S[i];
    std::vector<std::pair<ull, ull>> moved;
    while (!pairs.empty()) {
        bool have = false;
        ull bk = 0, bs = 0, bp = 0;
        for (const auto& kv : pairs) {
            const u32 lo = (u32)(kv.first >> B), hi = (u32)(kv.first & mask);
            const ull p = (ull)size[lo] * size[hi];
            if (!have || ksp_upgma_pair_before(kv.second, p, lo, hi, bs, bp, (u32)(bk >> B), (u32)(bk & mask))) { have = true; bk = kv.first; bs = kv.second; bp = p; }
        }
        const u32 lo = (u32)(bk >> B), hi = (u32)(bk & mask);
        rows.push_back(ksp_upgma_row{lo, hi, bs, size[lo], size[hi]});
        size[lo] += size[hi];
        pairs.erase(bk);
        moved.clear();
        for (auto it = pairs.begin(); it != pairs.end();) {
            const u32 a = (u32)(it->first >> B), b = (u32)(it->first & mask);
            if (a == hi || b == hi) {
                const u32 other = a == hi ? b : a;   // (never lo: that pair was the merged one)
                moved.emplace_back(((ull)std::min(lo, other) << B) | (ull)std::max(lo, other), it->second);
                it = pairs.erase(it);
            } else {
                ++it;
            }
        }
        for (const auto& kv : moved) pairs[kv.first] += kv.second;
    }
}

// bits of n_nodes - 1 (n_nodes >= 2): every node index fits
u32 node_bits(const u32 N) {
    u32 B = 1;
    while (B < 32 && ((u64)(N - 1) >> B)) ++B;
    return B;
}

// The tree on the CURRENT device over n > 0 edges and N > 1 nodes: the rows in merge order to `rows`.  Nothing of the caller's is
// written here.
int upgma_on_device(const char* who, const u32 N, const UpgmaIn& in, const u64 n, std::vector<ksp_upgma_row>& rows, ksp::UpgmaTrace& T) {
    int rc = KSP_OK;
    ksp::DeviceArena A;
    ksp::WorkgroupCap G;
    UpgmaBufs Bf;
    const u32 B = node_bits(N);
    const u64 n_chunks = chunks_of(n), tail = tail_pairs();
    const unsigned grid_nodes = (N + 255) / 256;
    ull h_c[kcWords] = {0};
    u64 live = 0, merges = 0;
    size_t tb = 0;
    if ((rc = ksp::workgroup_cap("KSP_UPGMA_MAX_WORKGROUPS", who, G))) return rc;
    if ((rc = scratch_bytes(n, 2 * B, &tb))) return rc;
    // ---- everything the call holds, sized and checked first: the formula of the header
    {
        const u64 bytes = 32 * n + 16 * (n_chunks + 1) + 40 * (u64)N + 8 * kcWords + (u64)tb;
        const std::string what = std::string("32 per record, 16 per 2 048 records, 40 per node, ") + std::to_string(tb) + " of sort and scan scratch";
        if ((rc = ksp::device_fits(who, bytes, what.c_str()))) return rc;
    }
    for (ull** p : {&Bf.key_a, &Bf.s_a, &Bf.key_b, &Bf.s_b})
        if ((rc = A.alloc(p, (size_t)n))) return rc;
    for (ull** p : {&Bf.chunk_count, &Bf.chunk_off})
        if ((rc = A.alloc(p, (size_t)(n_chunks + 1)))) return rc;
    if ((rc = A.alloc(&Bf.size, (size_t)N)) || (rc = A.alloc(&Bf.map, (size_t)N)) || (rc = A.alloc(&Bf.best, (size_t)N)) || (rc = A.alloc(&Bf.log, (size_t)N)) ||
        (rc = A.alloc(&Bf.counters, (size_t)kcWords)) || (rc = A.alloc_bytes(&Bf.tmp, tb)))
        return rc;
    Bf.tmp_bytes = tb;
    KSP_TRY_HIP(hipMemsetAsync(Bf.counters, 0, 8 * kcWords, nullptr));
    hipLaunchKernelGGL(k_upgma_init, dim3(grid_nodes), dim3(256), 0, nullptr, Bf.size, Bf.map, Bf.best, N);
    if (in.ed) hipLaunchKernelGGL(k_upgma_prep<true>, dim3(G.grid_of(n_chunks)), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, B, Bf.key_a, Bf.s_a, Bf.counters);
    else hipLaunchKernelGGL(k_upgma_prep<false>, dim3(G.grid_of(n_chunks)), dim3(kThreads), 0, nullptr, in, n, n_chunks, N, B, Bf.key_a, Bf.s_a, Bf.counters);
    KSP_TRY_HIP(hipGetLastError());
    // ---- the fold of the raw records: runs of any length
    if ((rc = sort_and_fold(Bf, A, G, n, B, false))) return rc;
    KSP_TRY_HIP(hipMemcpy(h_c, Bf.counters, 8 * kcWords, hipMemcpyDeviceToHost));
    if (h_c[kcDomain]) {
        ksp::set_error(std::string(who) + ": a record's value lies above 1 (a containment above 1: shared k-mers above a source's count)");
        return KSP_E_ARG;
    }
    live = h_c[kcLive];
    T.taking_part = h_c[kcTakingPart];
    T.first_pairs = live;
    if (live > n) { ksp::set_error(std::string(who) + ": more pairs than records"); return KSP_E_HIP; }
    // ---- the rounds
    while (live > 0 && !(tail && live <= tail)) {
        if (T.rounds >= (u64)N) { ksp::set_error(std::string(who) + ": more than " + std::to_string(N) + " rounds"); return KSP_E_HIP; }
        const u64 m_chunks = chunks_of(live);
        const unsigned grid = G.grid_of(m_chunks);
        hipLaunchKernelGGL(k_upgma_offer, dim3(grid), dim3(kThreads), 0, nullptr, (const ull*)Bf.key_a, (const ull*)Bf.s_a, live, m_chunks, (const u32*)Bf.size, B, Bf.best);
        hipLaunchKernelGGL(k_upgma_merge, dim3(grid), dim3(kThreads), 0, nullptr, (const ull*)Bf.key_a, (const ull*)Bf.s_a, live, m_chunks, (const ull*)Bf.best, B, Bf.size,
                           Bf.map, Bf.log, (u64)N - 1, Bf.counters);
        hipLaunchKernelGGL(k_upgma_relabel, dim3(grid), dim3(kThreads), 0, nullptr, Bf.key_a, live, m_chunks, (const u32*)Bf.map, B, Bf.best);
        KSP_TRY_HIP(hipGetLastError());
        if ((rc = sort_and_fold(Bf, A, G, live, B, true))) return rc;
        KSP_TRY_HIP(hipMemcpy(h_c, Bf.counters, 8 * kcWords, hipMemcpyDeviceToHost));   // the round's one read-back
        ++T.rounds;
        if (h_c[kcLogOverflow] || h_c[kcMerges] > (u64)N - 1) { ksp::set_error(std::string(who) + ": more merges than a forest has"); return KSP_E_HIP; }
        if (h_c[kcMerges] == merges) {
            ksp::set_error(std::string(who) + ": round " + std::to_string(T.rounds) + " merged nothing while " + std::to_string(live) + " pairs were live");
            return KSP_E_HIP;
        }
        if (h_c[kcLive] >= live) { ksp::set_error(std::string(who) + ": a round with a merge did not shorten the pair list"); return KSP_E_HIP; }
        merges = h_c[kcMerges];
        live = h_c[kcLive];
    }
    T.device_merges = merges;
    T.longest_run = h_c[kcLongestRun];
    T.handed_over = live;
    // ---- the log, the host finish, and the rows in the order
    rows.assign((size_t)merges, ksp_upgma_row());
    if (merges) KSP_TRY_HIP(hipMemcpy(rows.data(), Bf.log, (size_t)merges * sizeof(ksp_upgma_row), hipMemcpyDeviceToHost));
    if (live) {
        std::vector<ull> key((size_t)live), S((size_t)live);
        std::vector<u32> size((size_t)N);   // (all of it, 4 bytes per node: the roots of the list are a few of them)
        KSP_TRY_HIP(hipMemcpy(key.data(), Bf.key_a, (size_t)live * 8, hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipMemcpy(S.data(), Bf.s_a, (size_t)live * 8, hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipMemcpy(size.data(), Bf.size, (size_t)N * 4, hipMemcpyDeviceToHost));
        host_finish(key, S, size, B, rows);
    }
    T.host_merges = rows.size() - merges;
    if (rows.size() > (u64)N - 1) { ksp::set_error(std::string(who) + ": more merges than a forest has"); return KSP_E_HIP; }
    for (const ksp_upgma_row& r : rows)
        if (r.lo >= r.hi || r.hi >= N || !r.size_lo || !r.size_hi || !r.sum_q) { ksp::set_error(std::string(who) + ": a merge row is not a pair of clusters"); return KSP_E_HIP; }
    std::sort(rows.begin(), rows.end(), row_before);
done:
    return rc;
}

int check_upgma_args(const char* who, const u32 n_nodes, const u64 n_edges, const bool null_input, const ksp_upgma_row* h_rows, const u32* n_rows) {
    if (!n_rows || (n_nodes > 1 && !h_rows) || (n_edges && null_input)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (n_edges >= 0xFFFFFFFFull) { ksp::set_error(std::string(who) + ": 2^32 - 1 records or more (a sum of q would no longer fit 64 bits)"); return KSP_E_LIMIT; }
    return KSP_OK;
}

// the rows to the caller: only after the whole call has succeeded
void hand_out(const std::vector<ksp_upgma_row>& rows, ksp_upgma_row* h_rows, u32* n_rows) {
    std::copy(rows.begin(), rows.end(), h_rows);
    *n_rows = (u32)rows.size();
}

int upgma_edges(const char* who, const u32 n_nodes, const ksp_edge* d_edges, const u64 n_edges, const u32* d_cnt, const int col, ksp_upgma_row* h_rows, u32* n_rows,
                ksp::UpgmaTrace* trace) {
    ksp::UpgmaTrace T;
    std::vector<ksp_upgma_row> rows;
    int rc = KSP_OK;
    if (n_edges && n_nodes > 1) {   // (otherwise no kernel runs)
        UpgmaIn in;
        in.ed = d_edges; in.cnt = d_cnt; in.col = col;
        try {
            rc = upgma_on_device(who, n_nodes, in, n_edges, rows, T);
        } catch (const std::bad_alloc&) {
            ksp::set_error(std::string(who) + ": out of host memory");
            rc = KSP_E_LIMIT;
        }
    }
    g_trace = T;
    if (trace) *trace = T;
    if (rc == KSP_OK) hand_out(rows, h_rows, n_rows);
    return rc;
}

std::string g9(const double x) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.9g", x);
    return buf;
}

double row_average(const ksp_upgma_row& r) { return (double)r.sum_q / ((double)r.size_lo * (double)r.size_hi) / 4294967296.0; }

bool parse_u64(const std::string& t, u64& v) {   // decimal digits only
    const std::string s = strip(t);
    if (s.empty() || s.size() > 20) return false;
    for (const char c : s)
        if (c < '0' || c > '9') return false;
    errno = 0;
    char* end = nullptr;
    v = std::strtoull(s.c_str(), &end, 10);
    return !errno && end && *end == 0;
}

}  // namespace

namespace ksp {
int upgma_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, ksp_upgma_row* h_rows,
                          uint32_t* n_rows, UpgmaTrace* trace) {
    if (const int rc = check_upgma_args("upgma", n_nodes, n_edges, !d_edges || !d_cnt, h_rows, n_rows)) return rc;
    return upgma_edges("upgma", n_nodes, d_edges, n_edges, d_cnt, col, h_rows, n_rows, trace);
}

void write_upgma_files(const std::string& prefix, const std::string& dist, const std::vector<ksp_upgma_row>& rows, const std::vector<std::string>& name_of,
                       const bool newick) {
    std::string table = "source_1\tsource_2\t" + dist + "_average\tsum_q\tsize_1\tsize_2\tmerged_size\n";
    std::vector<TreeRow> tree_rows;
    for (const ksp_upgma_row& r : rows) {
        if (r.lo >= name_of.size() || r.hi >= name_of.size()) throw std::runtime_error("upgma: a merge names a node that is no row of .namesMap");
        const double avg = row_average(r);
        table += std::to_string((u64)r.lo + 1) + "\t" + std::to_string((u64)r.hi + 1) + "\t" + g9(avg) + "\t" + std::to_string(r.sum_q) + "\t" + std::to_string(r.size_lo) +
                 "\t" + std::to_string(r.size_hi) + "\t" + std::to_string((u64)r.size_lo + r.size_hi) + "\n";
        if (newick) tree_rows.push_back(TreeRow{r.lo, r.hi, avg, avg, std::string()});
    }
    auto exists = [](const std::string& path) { return (bool)std::ifstream(path); };
    const std::string tsv = prefix + "_kSpider_upgma_" + dist + ".tsv", nwk = prefix + "_kSpider_upgma_" + dist + ".newick";
    std::vector<std::string> created;
    try {
        if (!exists(tsv)) created.push_back(tsv);
        write_file_atomically(tsv, table);
        if (newick) {
            if (!exists(nwk)) created.push_back(nwk);
            std::ofstream f;
            PartialFiles files;
            files.open(nwk, f);
            write_newick(f, tree_rows, name_of);
            files.commit();
        }
    } catch (...) {
        for (const std::string& path : created) std::remove(path.c_str());
        throw;
    }
}
}  // namespace ksp

extern "C" int ksp_edges_upgma(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                               ksp_upgma_row* h_rows, uint32_t* n_rows) {
    const char* who = "ksp_edges_upgma";
    if (const int rc = check_upgma_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, h_rows, n_rows)) return rc;
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return upgma_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, h_rows, n_rows, nullptr);
}

extern "C" int ksp_upgma_valued(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const float* h_value, uint64_t n_edges,
                                ksp_upgma_row* h_rows, uint32_t* n_rows) {
    const char* who = "ksp_upgma_valued";
    if (const int rc = check_upgma_args(who, n_nodes, n_edges, !h_a || !h_b || !h_value, h_rows, n_rows)) return rc;
    for (u64 e = 0; e < n_edges; ++e) {
        if (h_a[e] >= n_nodes || h_b[e] >= n_nodes) { ksp::set_error(std::string(who) + ": node index out of range"); return KSP_E_ARG; }
        if (h_value[e] < 0 || h_value[e] > 1) { ksp::set_error(std::string(who) + ": a value lies outside [0, 1]"); return KSP_E_ARG; }
    }
    if (const int rc = ksp::set_device(who, device)) return rc;
    ksp::UpgmaTrace T;
    g_trace = T;
    if (n_edges == 0 || n_nodes <= 1) { *n_rows = 0; return KSP_OK; }
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_a = nullptr, *d_b = nullptr;
    float* d_val = nullptr;
    UpgmaIn in;
    std::vector<ksp_upgma_row> rows;
    if ((rc = ksp::device_fits(who, 12ull * n_edges, "12 per valued edge"))) return rc;   // (the rest is asked for once these are up)
    if ((rc = ksp::upload_pairs(A, h_a, h_b, n_edges, &d_a, &d_b)) || (rc = A.alloc(&d_val, (size_t)n_edges))) return rc;
    KSP_TRY_HIP(hipMemcpy(d_val, h_value, (size_t)n_edges * 4, hipMemcpyHostToDevice));
    in.a = d_a; in.b = d_b; in.val = d_val;
    try {
        rc = upgma_on_device(who, n_nodes, in, n_edges, rows, T);
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        rc = KSP_E_LIMIT;
    }
    g_trace = T;
    if (rc == KSP_OK) hand_out(rows, h_rows, n_rows);
done:
    return rc;
}

extern "C" int ksp_upgma_before(uint64_t s1, uint32_t size_lo1, uint32_t size_hi1, uint32_t lo1, uint32_t hi1, uint64_t s2, uint32_t size_lo2, uint32_t size_hi2,
                                uint32_t lo2, uint32_t hi2, int* before) {
    if (!before) { ksp::set_error("ksp_upgma_before: NULL argument"); return KSP_E_ARG; }
    if (!size_lo1 || !size_hi1 || !size_lo2 || !size_hi2) { ksp::set_error("ksp_upgma_before: a cluster of size 0"); return KSP_E_ARG; }
    *before = ksp_upgma_pair_before(s1, (u64)size_lo1 * size_hi1, lo1, hi1, s2, (u64)size_lo2 * size_hi2, lo2, hi2) ? 1 : 0;
    return KSP_OK;
}

extern "C" int ksp_debug_upgma_counts(uint64_t out[6]) {
    if (!out) { ksp::set_error("ksp_debug_upgma_counts: NULL argument"); return KSP_E_ARG; }
    out[0] = g_trace.first_pairs;
    out[1] = g_trace.rounds;
    out[2] = g_trace.device_merges;
    out[3] = g_trace.handed_over;
    out[4] = g_trace.host_merges;
    out[5] = g_trace.longest_run;
    return KSP_OK;
}

// (tools/upgma_times.py) HIP-event times of `reps` runs of ksp_edges_upgma's device part and host finish over the same records:
// each time covers everything the call does, its allocations and copies included.  ms[reps]; counts: ksp_debug_upgma_counts of the last run.
extern "C" int ksp_debug_upgma_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, int reps,
                                     float* ms, ksp_upgma_row* h_rows, uint32_t* n_rows, uint64_t counts[6]) {
    const char* who = "ksp_debug_upgma_times";
    if (!ms || reps < 1 || !counts || !n_nodes || dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": bad argument"); return KSP_E_ARG; }
    if (const int rc = check_upgma_args(who, n_nodes, n_edges, !d_edges || !d_kmer_counts, h_rows, n_rows)) return rc;
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if ((rc = upgma_edges(who, n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, h_rows, n_rows, nullptr))) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
    }
    rc = ksp_debug_upgma_counts(counts);
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}

// ---- the file drivers --------------------------------------------------------------------------------------------------------------

extern "C" int kspider_upgma(const char* index_prefix, const char* dist_type, int newick) {
    const char* who = "kspider_upgma";
    if (!index_prefix) { ksp::set_error(std::string(who) + ": index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (col < 3 || col > 5) {
        ksp::set_error(std::string(who) + ": distance '" + dt + "' is not min_cont, avg_cont or max_cont (an average is one of containments in [0, 1])");
        return KSP_E_ARG;
    }
    g_trace = ksp::UpgmaTrace();
    try {
        std::vector<std::string> name_of;
        std::vector<u32> ea, eb;
        std::vector<float> value;
        read_cluster_inputs(prefix, col, name_of, [&](const long long a, const long long b, const double, const std::string& t) {
            const float v = std::strtof(t.c_str(), nullptr);
            if (v != v || a == b || (v >= 0 && (double)v * 4294967296.0 < 1.0)) return;   // takes no part: its ids are not looked at
            ksp::check_row_nodes(a, b, name_of.size());
            ea.push_back((u32)(a - 1));
            eb.push_back((u32)(b - 1));
            value.push_back(v);   // (one outside [0, 1] is refused by the call below, before any file is written)
        });
        const u64 N = name_of.size();
        if (N >= 0xFFFFFFFFull) throw std::runtime_error("more than 2^32 - 2 names");
        std::vector<ksp_upgma_row> rows((size_t)N + 1);
        u32 n_rows = 0;
        const int rc = ksp_upgma_valued(ksp::device_from_env(), (u32)N, ea.data(), eb.data(), value.data(), ea.size(), rows.data(), &n_rows);
        if (rc) return rc;
        rows.resize(n_rows);
        ksp::write_upgma_files(prefix, dt, rows, name_of, newick != 0);
        if (std::getenv("KSPIDER_VERBOSE"))
            std::cout << "kspider_amd: upgma: " << g_trace.taking_part << " records taking part, " << g_trace.first_pairs << " pairs, " << g_trace.rounds
                      << " device rounds, merges " << g_trace.device_merges << " on the device / " << g_trace.host_merges << " by the host finish" << std::endl;
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}

extern "C" int kspider_cluster_from_upgma(const char* index_prefix, const char* dist_type, double cutoff) {
    const char* who = "kspider_cluster_from_upgma";
    if (!index_prefix) { ksp::set_error(std::string(who) + ": index_prefix is NULL"); return KSP_E_ARG; }
    const std::string prefix = index_prefix, dt = dist_type && *dist_type ? dist_type : "max_cont";
    const int col = cluster_col(dt);
    if (col < 3 || col > 5) { ksp::set_error(std::string(who) + ": distance '" + dt + "' is not min_cont, avg_cont or max_cont"); return KSP_E_ARG; }
    if (!(cutoff >= 0 && cutoff <= 1)) { ksp::set_error(std::string(who) + ": the cut-off is not in [0, 1]"); return KSP_E_ARG; }
    const u64 q_cut = (u64)(cutoff * 4294967296.0);
    try {
        std::vector<std::string> name_of;
        ksp::read_names_map(prefix, name_of);
        const u64 N = name_of.size();
        const std::string path = prefix + "_kSpider_upgma_" + dt + ".tsv";
        std::ifstream f(path);
        if (!f) throw std::runtime_error("cannot open " + path);
        TreeDsu dsu(N);
        std::string line;
        std::vector<std::string> p;
        if (!std::getline(f, line)) throw std::runtime_error("no header in " + path);
        while (std::getline(f, line)) {
            split_tabs(strip(line), p);
            long long a, b;
            u64 sum_q, s1, s2;
            if (p.size() < 6 || !parse_id(p[0], a) || !parse_id(p[1], b) || !parse_u64(p[3], sum_q) || !parse_u64(p[4], s1) || !parse_u64(p[5], s2) || !s1 || !s2 ||
                s1 > 0xFFFFFFFFull || s2 > 0xFFFFFFFFull)
                throw std::runtime_error("malformed row in " + path);
            ksp::check_row_nodes(a, b, N);
            if ((unsigned __int128)sum_q < (unsigned __int128)q_cut * (s1 * s2)) continue;   // average below the cut-off, exactly
            const u32 ra = dsu.find((u32)(a - 1)), rb = dsu.find((u32)(b - 1));
            if (ra != rb) dsu.parent[std::max(ra, rb)] = std::min(ra, rb);
        }
        std::vector<u32> label((size_t)N);
        for (u64 v = 0; v < N; ++v) label[(size_t)v] = dsu.find((u32)v);
        ksp::write_cluster_file_as(prefix + "_kSpider_clusters_upgma_" + dt + "_" + py_float_repr(cutoff * 100.0) + "%.tsv", label, name_of);
        return KSP_OK;
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    } catch (const std::exception& e) {
        ksp::set_error(std::string(who) + ": " + e.what());
        return KSP_E_IO;
    }
}
