// The cut-off ladder: the connected components of the join's edges at a list of K cut-offs, from ONE classification of the
// edges and ONE components computation that is continued from cut-off to cut-off, not restarted.
//
// The clusterings of a ladder are nested.  Order the cut-offs by strictness (mode-0 critical floats of ksp::cc_critical
// ascending, then the mode-1 ones, which only a NaN passes): the cut-offs an edge passes are the L least strict ones, L is
// the edge's LEVEL (0..K, a NaN has K), and the clustering at strictness rank r is the components of the edges with L > r.
//   level     k_sweep_level: the column value of every record once (edge_col_value), its level as the upper bound of the
//             value in the table of critical floats (LDS), one byte per record, a histogram of the K + 1 levels
//   bands     the host turns the histogram into band offsets: band l = the edges of level l, l = 1..K
//   scatter   k_sweep_scatter: the endpoints of every edge of level >= 1 into its band, as a[] / b[] (8 bytes per edge)
//   ranks     for r = K - 1 down to 0: hook over band r + 1 only, on the parent[] the ranks above left; snapshot
// Both passes own chunks of kSweepChunkEdges consecutive records per workgroup, as the containment cut does (cut.hip), and
// no workgroup ever waits on another.  Every count, offset and index is 64-bit.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/kspider_amd.h"
#include "cc_kernels.hip.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kSweepChunkEdges = KSP_SWEEP_CHUNK_EDGES;   // (the reasons for 2 048 records per 256 threads: cut.hip)
constexpr int kSweepThreads = 256;
constexpr int kSweepIters = (int)(kSweepChunkEdges / kSweepThreads);   // records per lane and chunk
constexpr u32 kSweepLevels = KSP_SWEEP_MAX_CUTOFFS + 1;                // levels 0..255: one per thread of a workgroup
static_assert(kSweepIters * kSweepThreads == (int)kSweepChunkEdges && kSweepLevels == (u32)kSweepThreads, "a chunk is whole ballots; a level per thread");

// first record of wave `wave` in chunk `chunk`: wave w owns the records [w * 512, (w + 1) * 512) of its chunk
__device__ inline u64 sweep_wave_base(const u64 chunk, const u32 wave) { return chunk * kSweepChunkEdges + (u64)wave * (kSweepIters * 64); }

// what the host and the two kernels share (device memory): one allocation, one upload
struct SweepMeta {
    unsigned long long hist[kSweepLevels];     // edges per level (k_sweep_level adds, the host reads)
    unsigned long long cursor[kSweepLevels];   // next free position of band l (the host sets the band offsets, k_sweep_scatter adds)
    float crit[kSweepLevels];                  // the n0 mode-0 critical floats, ascending
    u32 changed[4];                            // [0] a hook changed a parent, [1] the last jump did, [2] any other jump
};

// Level of every record and the histogram of the levels.  The level of a value v is the number of cut-offs it passes: NaN
// passes all K; any other v passes the mode-0 cut-offs whose critical float is not above it — !(v < crit) — and no mode-1
// cut-off, so it is the upper bound of v in the ascending table.
__global__ __launch_bounds__(kSweepThreads) void k_sweep_level(const ksp_edge* __restrict__ ed, const u64 n, const u64 n_chunks, const u32* __restrict__ cnt,
                                                               const int col, const SweepMeta* __restrict__ meta, const u32 n0, const u32 K,
                                                               uint8_t* __restrict__ level, unsigned long long* __restrict__ hist) {
    __shared__ float s_crit[kSweepLevels];
    __shared__ u32 s_hist[kSweepLevels];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s_crit[threadIdx.x] = threadIdx.x < n0 ? meta->crit[threadIdx.x] : 0.0f;
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    u32 since_flush = 0;   // chunks in s_hist: flushed before 2^31 records could overflow a 32-bit counter
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = sweep_wave_base(chunk, wave);
        ksp_edge x[kSweepIters];
#pragma unroll
        for (int k = 0; k < kSweepIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e < n) x[k] = ed[e];
        }
#pragma unroll
        for (int k = 0; k < kSweepIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e >= n) continue;
            const float v = edge_col_value(x[k], cnt, col);
            u32 l = 0;
            if (v != v) l = K;
            else {
#pragma unroll
                for (u32 step = kSweepLevels / 2; step; step >>= 1)   // upper bound: entries [0, l) are <= v
                    if (l + step <= n0 && !(v < s_crit[l + step - 1])) l += step;
            }
            level[e] = (uint8_t)l;
            atomicAdd(&s_hist[l], 1u);
        }
        if (++since_flush == (1u << 20)) {
            __syncthreads();
            if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
            s_hist[threadIdx.x] = 0;
            since_flush = 0;
            __syncthreads();
        }
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);   // one per non-empty level and workgroup
}

// the two input forms of the scatter: the join's records (the endpoints are the first 8 bytes of a record) or host-classified a[] / b[]
struct SweepRecords {
    const ksp_edge* __restrict__ ed;
    __device__ uint2 ends(const u64 e) const { return *reinterpret_cast<const uint2*>(ed + e); }
};
struct SweepArrays {
    const u32* __restrict__ a;
    const u32* __restrict__ b;
    __device__ uint2 ends(const u64 e) const { return make_uint2(a[e], b[e]); }
};

// The endpoints of every edge of level l >= 1 into band l.  Per chunk: positions inside the chunk's share of each band by
// wave-aggregated LDS atomics (per ballot, one atomic per distinct level present in the wave: its first lane adds the
// popcount, every lane of that level takes its rank among them), then one global atomicAdd per non-empty band reserves the
// chunk's range, then the stores.  The order inside a band depends on which chunk reserves first: the labels do not.
template <class In>
__global__ __launch_bounds__(kSweepThreads) void k_sweep_scatter(const In in, const uint8_t* __restrict__ level, const u64 n, const u64 n_chunks,
                                                                 unsigned long long* __restrict__ cursor, u32* __restrict__ out_a, u32* __restrict__ out_b) {
    __shared__ u32 s_count[kSweepLevels];
    __shared__ unsigned long long s_base[kSweepLevels];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = sweep_wave_base(chunk, wave);
        s_count[threadIdx.x] = 0;
        u32 l[kSweepIters], pos[kSweepIters];
        uint2 x[kSweepIters];
#pragma unroll
        for (int k = 0; k < kSweepIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            l[k] = e < n ? level[e] : 0u;
            x[k] = e < n ? in.ends(e) : make_uint2(0, 0);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSweepIters; ++k) {
            pos[k] = 0;
            unsigned long long todo = __ballot(l[k] != 0);
            while (todo) {   // (uniform: a ballot) one trip per distinct level among the 64 records
                const int first = __ffsll(todo) - 1;
                const u32 lv = (u32)__builtin_amdgcn_readlane((int)l[k], first);
                const unsigned long long same = __ballot(l[k] == lv);
                u32 start = 0;
                if ((int)lane == first) start = atomicAdd(&s_count[lv], (u32)__popcll(same));
                start = (u32)__builtin_amdgcn_readlane((int)start, first);
                if (l[k] == lv) pos[k] = start + __builtin_amdgcn_mbcnt_hi((u32)(same >> 32), __builtin_amdgcn_mbcnt_lo((u32)same, 0u));
                todo &= ~same;
            }
        }
        __syncthreads();
        if (threadIdx.x && s_count[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
        __syncthreads();   // (s_count is cleared for the next chunk only behind this barrier, s_base written only behind the next one)
#pragma unroll
        for (int k = 0; k < kSweepIters; ++k)
            if (l[k]) {
                const u64 at = s_base[l[k]] + pos[k];
                out_a[at] = x[k].x;
                out_b[at] = x[k].y;
            }
    }
}

// The ladder of one call: the cut-offs in order of strictness.
struct Ladder {
    u32 K = 0, n0 = 0;                // cut-offs; those of mode 0
    float crit[kSweepLevels] = {};    // critical floats of ranks 0 .. n0 - 1, ascending
    u32 caller_of[kSweepLevels] = {}; // rank -> index in the caller's list
};
void make_ladder(const double* cutoffs, const u32 K, Ladder& L) {
    std::vector<float> vcrit(K);
    std::vector<int> mode(K);
    for (u32 i = 0; i < K; ++i) ksp::cc_critical(cutoffs[i], &vcrit[i], &mode[i]);
    std::vector<u32> order(K);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](const u32 x, const u32 y) { return mode[x] != mode[y] ? mode[x] < mode[y] : (!mode[x] && vcrit[x] < vcrit[y]); });
    L.K = K;
    L.n0 = 0;
    for (u32 r = 0; r < K; ++r) {
        L.caller_of[r] = order[r];
        if (!mode[order[r]]) L.crit[L.n0++] = vcrit[order[r]];
    }
}

// workgroups of both passes: one per chunk up to 8 per CU, the rest by the chunk loop; $KSP_SWEEP_MAX_WORKGROUPS (tests)
int sweep_grid(const u64 n_chunks, unsigned* grid) {
    ksp::WorkgroupCap g;
    if (const int rc = ksp::workgroup_cap("KSP_SWEEP_MAX_WORKGROUPS", "sweep", g)) return rc;
    *grid = g.grid_of(n_chunks);
    return KSP_OK;
}

// band offsets from the histogram: band l = [off[l - 1], off[l]), l = 1..K; off[K] = the edges of level >= 1
void band_offsets(const unsigned long long* hist, const u32 K, u64* off, unsigned long long* cursor) {
    off[0] = 0;
    cursor[0] = 0;
    for (u32 l = 1; l <= K; ++l) {
        cursor[l] = off[l - 1];
        off[l] = off[l - 1] + hist[l];
    }
}

// Levels and histogram of the records on the CURRENT device: d_level[n], h_hist[K + 1].  d_meta is written here.
int level_on_device(const ksp_edge* d_edges, const u64 n, const u32* d_cnt, const int col, const Ladder& L, SweepMeta* d_meta,
                    uint8_t* d_level, unsigned long long* h_hist) {
    int rc = KSP_OK;
    unsigned grid = 1;
    const u64 n_chunks = (n + kSweepChunkEdges - 1) / kSweepChunkEdges;
    std::vector<SweepMeta> hm(1);
    std::memset(hm.data(), 0, sizeof(SweepMeta));
    std::memcpy(hm[0].crit, L.crit, sizeof(float) * L.n0);
    std::fill(h_hist, h_hist + L.K + 1, 0ull);
    KSP_TRY_HIP(hipMemcpy(d_meta, hm.data(), sizeof(SweepMeta), hipMemcpyHostToDevice));
    if (n == 0) return KSP_OK;
    if ((rc = sweep_grid(n_chunks, &grid))) return rc;
    hipLaunchKernelGGL(k_sweep_level, dim3(grid), dim3(kSweepThreads), 0, nullptr, d_edges, n, n_chunks, d_cnt, col, (const SweepMeta*)d_meta, L.n0, L.K, d_level,
                       d_meta->hist);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(hipMemcpy(h_hist, d_meta->hist, sizeof(unsigned long long) * (L.K + 1), hipMemcpyDeviceToHost));
done:
    return rc;
}

// The edges of level >= 1 into their bands on the CURRENT device; h_cursor[K + 1] = the band offsets (band_offsets).
template <class In>
int scatter_on_device(const In in, const uint8_t* d_level, const u64 n, const u32 K, const unsigned long long* h_cursor, SweepMeta* d_meta, u32* d_a, u32* d_b) {
    int rc = KSP_OK;
    unsigned grid = 1;
    const u64 n_chunks = (n + kSweepChunkEdges - 1) / kSweepChunkEdges;
    if (n == 0) return KSP_OK;
    if ((rc = sweep_grid(n_chunks, &grid))) return rc;
    KSP_TRY_HIP(hipMemcpy(d_meta->cursor, h_cursor, sizeof(unsigned long long) * (K + 1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_sweep_scatter<In>, dim3(grid), dim3(kSweepThreads), 0, nullptr, in, d_level, n, n_chunks, d_meta->cursor, d_a, d_b);
    KSP_TRY_HIP(hipGetLastError());
done:
    return rc;
}

// The components of every rank from the banded edges: d_rows[row_of_rank[r] * N ..] = labels of rank r (device memory).
int ranks_on_device(const u32 N, const u32* d_a, const u32* d_b, const u64* off, const u32 K, const u32* row_of_rank, SweepMeta* d_meta, u32* d_parent,
                    u32* d_rows) {
    int rc = KSP_OK;
    const unsigned gn = (N + 255) / 256;
    u32* d_changed = d_meta->changed;
    hipLaunchKernelGGL(k_cc_init, dim3(gn), dim3(256), 0, nullptr, d_parent, N);
    KSP_TRY_HIP(hipGetLastError());
    // Why continuing on the parent[] of the ranks above is sound, although their edges are never looked at again.
    //   * Before every hook pass every tree is a star: true at the start, and below no hook pass starts before a jump pass
    //     has found nothing left to do.
    //   * So every label a hook pass reads — parent[x] of an endpoint x — is a node that was a root when the pass began (a
    //     leaf's parent is such a root and does not change during the pass; a root's parent is itself or a label some edge
    //     lowered it to).  A hook therefore only ever re-parents roots: a node that was a leaf keeps its parent.
    //   * After the pass the leaves still point to their root and the roots to smaller roots; the jump passes flatten that, so
    //     every member of a star ends under the root of its own root.  A component of an earlier rank, which is a star here,
    //     is never separated.  (Two jump passes per round do NOT flatten a chain of four hooked roots or more: hooking again
    //     at that point can re-parent a non-root whose former leaves have already jumped past it, and with the edges that
    //     joined them no longer examined they would stay apart.  Hence the jump passes go on until one changes nothing.)
    //   * A link lost inside one hook pass — atomicMin lowered parent[R] from Y to a smaller label — is re-made: the band edge
    //     that proposed Y is examined again every round and finds two different labels as long as the two trees are apart.
    //   * When a hook pass changes nothing every edge of the band joins two nodes of one star, and every link ever made was
    //     proposed by an edge between the two trees: the stars are the components of the bands so far.
    for (u32 r = K; r-- > 0;) {
        const u64 lo = off[r], m = off[r + 1] - off[r];   // band r + 1; an empty band costs no round
        if (m) {
            const unsigned ge = (unsigned)std::min<u64>((m + 255) / 256, 1u << 16);
            u32 h_changed[2] = {1, 0};
            for (int round = 0; h_changed[0] && round < 10000; ++round) {
                KSP_TRY_HIP(hipMemsetAsync(d_changed, 0, 16, nullptr));
                hipLaunchKernelGGL(k_cc_hook, dim3(ge), dim3(256), 0, nullptr, d_a + lo, d_b + lo, m, d_parent, d_changed);
                h_changed[1] = 1;
                for (int flat = 0; h_changed[1] && flat < 64; ++flat) {
                    if (flat) KSP_TRY_HIP(hipMemsetAsync(d_changed + 1, 0, 4, nullptr));
                    hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, N, d_changed + 2);
                    hipLaunchKernelGGL(k_cc_jump, dim3(gn), dim3(256), 0, nullptr, d_parent, N, d_changed + 1);
                    KSP_TRY_HIP(hipMemcpy(h_changed, d_changed, 8, hipMemcpyDeviceToHost));
                }
                if (h_changed[1]) { ksp::set_error("sweep: the trees did not flatten"); rc = KSP_E_HIP; goto done; }
            }
            if (h_changed[0]) { ksp::set_error("sweep: did not converge"); rc = KSP_E_HIP; goto done; }
        }
        KSP_TRY_HIP(hipMemcpyAsync(d_rows + (u64)row_of_rank[r] * N, d_parent, (size_t)N * 4, hipMemcpyDeviceToDevice, nullptr));
    }
done:
    return rc;
}

int check_sweep_args(const char* who, const ksp_edge* d_edges, const u64 n_edges, const u32* d_kmer_counts, const int dist_col, const double* cutoffs,
                     const u32 n_cutoffs) {
    if (!cutoffs || n_cutoffs < 1 || n_cutoffs > KSP_SWEEP_MAX_CUTOFFS) {
        ksp::set_error(std::string(who) + ": between 1 and " + std::to_string(KSP_SWEEP_MAX_CUTOFFS) + " cut-offs");
        return KSP_E_ARG;
    }
    if (n_edges && (!d_edges || !d_kmer_counts)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    for (u32 i = 0; i < n_cutoffs; ++i)
        if (cutoffs[i] != cutoffs[i]) { ksp::set_error(std::string(who) + ": a cut-off is NaN"); return KSP_E_ARG; }
    return KSP_OK;
}

// what one call holds on the device (memory of the call's DeviceArena)
struct SweepBufs {
    SweepMeta* meta = nullptr;
    uint8_t* level = nullptr;
    u32 *a = nullptr, *b = nullptr, *parent = nullptr, *rows = nullptr;
    u32 *in_a = nullptr, *in_b = nullptr;   // (host-classified form: the uploaded lists)
};

}  // namespace

namespace ksp {
// ksp_components_edges_sweep on the CURRENT device (h_labels: n_cutoffs x n_nodes in the caller's order; h_kept may be NULL)
int sweep_edges_on_device(const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col,
                          const double* cutoffs, const uint32_t n_cutoffs, uint32_t* h_labels, uint64_t* h_kept) {
    int rc = KSP_OK;
    const u32 N = n_nodes, K = n_cutoffs;
    Ladder L;
    SweepBufs B;
    ksp::DeviceArena A;
    unsigned long long hist[kSweepLevels] = {}, cursor[kSweepLevels] = {};
    u64 off[kSweepLevels] = {};
    make_ladder(cutoffs, K, L);
    if ((rc = device_fits("sweep", (u64)sizeof(SweepMeta) + n_edges + ((u64)K + 1) * N * 4, ""))) return rc;
    if ((rc = A.alloc(&B.meta, 1))) goto done;
    if (n_edges && (rc = A.alloc(&B.level, (size_t)n_edges))) goto done;
    if ((rc = level_on_device(d_edges, n_edges, d_cnt, col, L, B.meta, B.level, hist))) goto done;
    band_offsets(hist, K, off, cursor);
    if ((rc = device_fits("sweep", off[K] * 8 + ((u64)K + 1) * N * 4, ""))) goto done;
    if (off[K]) {
        if ((rc = A.alloc(&B.a, (size_t)off[K])) || (rc = A.alloc(&B.b, (size_t)off[K]))) goto done;
        if ((rc = scatter_on_device(SweepRecords{d_edges}, B.level, n_edges, K, cursor, B.meta, B.a, B.b))) goto done;
    }
    if (N) {
        if ((rc = A.alloc(&B.parent, (size_t)N)) || (rc = A.alloc(&B.rows, (size_t)K * N))) goto done;
        if ((rc = ranks_on_device(N, B.a, B.b, off, K, L.caller_of, B.meta, B.parent, B.rows))) goto done;
        KSP_TRY_HIP(hipMemcpy(h_labels, B.rows, (size_t)K * N * 4, hipMemcpyDeviceToHost));
    } else {
        KSP_TRY_HIP(hipDeviceSynchronize());
    }
    if (h_kept)
        for (u32 r = 0; r < K; ++r) h_kept[L.caller_of[r]] = off[K] - off[r];   // the edges of level > r
done:
    return rc;
}
}  // namespace ksp

extern "C" int ksp_components_edges_sweep(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                                          int dist_col, const double* cutoffs, uint32_t n_cutoffs, uint32_t* h_labels, uint64_t* h_kept) {
    if (const int rc = check_sweep_args("ksp_components_edges_sweep", d_edges, n_edges, d_kmer_counts, dist_col, cutoffs, n_cutoffs)) return rc;
    if (n_nodes && !h_labels) { ksp::set_error("ksp_components_edges_sweep: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_components_edges_sweep", device)) return rc;
    return ksp::sweep_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoffs, n_cutoffs, h_labels, h_kept);
}

extern "C" int ksp_components_sweep(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint8_t* h_level, uint64_t n_edges,
                                    uint32_t n_levels, uint32_t* h_labels) {
    if (n_levels < 1 || n_levels > KSP_SWEEP_MAX_CUTOFFS) {
        ksp::set_error("ksp_components_sweep: between 1 and " + std::to_string(KSP_SWEEP_MAX_CUTOFFS) + " levels");
        return KSP_E_ARG;
    }
    if ((n_edges && (!h_a || !h_b || !h_level)) || (n_nodes && !h_labels)) { ksp::set_error("ksp_components_sweep: NULL argument"); return KSP_E_ARG; }
    const u32 N = n_nodes, K = n_levels;
    unsigned long long hist[kSweepLevels] = {}, cursor[kSweepLevels] = {};
    u64 off[kSweepLevels] = {};
    for (u64 e = 0; e < n_edges; ++e) {
        if (h_level[e] > K) { ksp::set_error("ksp_components_sweep: a level above n_levels"); return KSP_E_ARG; }
        if (h_level[e] && (h_a[e] >= N || h_b[e] >= N)) { ksp::set_error("ksp_components_sweep: node index out of range"); return KSP_E_ARG; }
        ++hist[h_level[e]];
    }
    if (const int rc = ksp::set_device("ksp_components_sweep", device)) return rc;
    if (N == 0) return KSP_OK;
    int rc = KSP_OK;
    SweepBufs B;
    ksp::DeviceArena A;
    std::vector<u32> row_of_rank(K);
    std::iota(row_of_rank.begin(), row_of_rank.end(), 0u);
    band_offsets(hist, K, off, cursor);
    if ((rc = ksp::device_fits("ksp_components_sweep", (u64)sizeof(SweepMeta) + n_edges * 9 + off[K] * 8 + ((u64)K + 1) * N * 4, ""))) return rc;
    if ((rc = A.alloc(&B.meta, 1))) goto done;
    KSP_TRY_HIP(hipMemset(B.meta, 0, sizeof(SweepMeta)));
    if (off[K]) {
        if ((rc = ksp::upload_pairs(A, h_a, h_b, n_edges, &B.in_a, &B.in_b))) goto done;
        if ((rc = A.alloc(&B.level, (size_t)n_edges)) || (rc = A.alloc(&B.a, (size_t)off[K])) || (rc = A.alloc(&B.b, (size_t)off[K]))) goto done;
        KSP_TRY_HIP(hipMemcpy(B.level, h_level, (size_t)n_edges, hipMemcpyHostToDevice));
        if ((rc = scatter_on_device(SweepArrays{B.in_a, B.in_b}, B.level, n_edges, K, cursor, B.meta, B.a, B.b))) goto done;
    }
    if ((rc = A.alloc(&B.parent, (size_t)N)) || (rc = A.alloc(&B.rows, (size_t)K * N))) goto done;
    if ((rc = ranks_on_device(N, B.a, B.b, off, K, row_of_rank.data(), B.meta, B.parent, B.rows))) goto done;
    KSP_TRY_HIP(hipMemcpy(h_labels, B.rows, (size_t)K * N * 4, hipMemcpyDeviceToHost));
done:
    return rc;
}

// (tests) the two kernels without the components: d_level[n_edges] (device) = the level of every record, levels counted in
// order of strictness; h_band_off[n_cutoffs + 1]: band l = [h_band_off[l - 1], h_band_off[l]) of d_a / d_b (device, room for
// the edges of level >= 1; at most n_edges), which hold the endpoints of the edges of level l in any order.
extern "C" int ksp_debug_sweep_bands(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                                     const double* cutoffs, uint32_t n_cutoffs, uint8_t* d_level, uint64_t* h_band_off, uint32_t* d_a, uint32_t* d_b) {
    if (const int rc = check_sweep_args("ksp_debug_sweep_bands", d_edges, n_edges, d_kmer_counts, dist_col, cutoffs, n_cutoffs)) return rc;
    if (!h_band_off || (n_edges && (!d_level || !d_a || !d_b))) { ksp::set_error("ksp_debug_sweep_bands: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_debug_sweep_bands", device)) return rc;
    int rc = KSP_OK;
    Ladder L;
    SweepBufs B;
    ksp::DeviceArena A;
    unsigned long long hist[kSweepLevels] = {}, cursor[kSweepLevels] = {};
    u64 off[kSweepLevels] = {};
    make_ladder(cutoffs, n_cutoffs, L);
    if ((rc = A.alloc(&B.meta, 1))) goto done;
    if ((rc = level_on_device(d_edges, n_edges, d_kmer_counts, dist_col, L, B.meta, d_level, hist))) goto done;
    band_offsets(hist, n_cutoffs, off, cursor);
    if (off[n_cutoffs] && (rc = scatter_on_device(SweepRecords{d_edges}, d_level, n_edges, n_cutoffs, cursor, B.meta, d_a, d_b))) goto done;
    KSP_TRY_HIP(hipDeviceSynchronize());
    std::copy(off, off + n_cutoffs + 1, h_band_off);
done:
    return rc;
}

// (tools/sweep_times.py) HIP-event times of `reps` runs of one way to get the labels of every cut-off over the same records:
// which 0 = ksp_components_edges_sweep, 1 = one ksp_components_edges per cut-off.  Each time covers everything the calls do
// on the device, their allocations and copies to the host included.  ms[reps]; h_labels: n_cutoffs x n_nodes.
extern "C" int ksp_debug_sweep_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                                     int dist_col, const double* cutoffs, uint32_t n_cutoffs, int which, int reps, float* ms, uint32_t* h_labels) {
    if (!ms || reps < 1 || which < 0 || which > 1 || !h_labels || !n_nodes) { ksp::set_error("ksp_debug_sweep_times: bad argument"); return KSP_E_ARG; }
    if (const int rc = check_sweep_args("ksp_debug_sweep_times", d_edges, n_edges, d_kmer_counts, dist_col, cutoffs, n_cutoffs)) return rc;
    if (const int rc = ksp::set_device("ksp_debug_sweep_times", device)) return rc;
    int rc = KSP_OK;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    for (int r = 0; r < reps; ++r) {
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if (which == 0) rc = ksp::sweep_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoffs, n_cutoffs, h_labels, nullptr);
        else
            for (u32 i = 0; i < n_cutoffs && !rc; ++i)
                rc = ksp::cc_edges_on_device(n_nodes, d_edges, n_edges, d_kmer_counts, dist_col, cutoffs[i], h_labels + (u64)i * n_nodes, nullptr);
        if (rc) goto done;
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}
