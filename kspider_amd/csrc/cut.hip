// The containment cut: a STABLE compaction of the join's ksp_edge records by the reference's clustering test
// (cc_edge_kept, edge_cut.hip.h: one compare against the critical float of ksp::cc_critical), on the device, before the
// records are gathered, sorted, copied to the host and printed.
//
// Three passes, ordered by kernel boundaries alone — no workgroup ever waits on another:
//   count    a workgroup owns chunks of kCutChunkEdges consecutive records; every wave takes one ballot of the predicate per
//            64 records and adds up the popcounts; one 64-bit count per chunk
//   scan     exclusive scan of the chunk counts (rocPRIM): the chunk offsets and, behind the last chunk, the total
//   scatter  the same chunks again: a record goes to chunk offset + kept records of the waves before mine in the chunk (LDS)
//            + kept records of my wave before this ballot + popcount of the ballot below my lane
// Inside a chunk wave w owns the records [w * 512, (w + 1) * 512): the order of the records is (chunk, wave, ballot, lane),
// which is the order of the positions, so the kept records keep their input order.
// The scatter pass either evaluates the predicate again or reads the ballots the count pass left (8 bytes per 64 records);
// with the ballots a lane loads its record only when it is kept.  Every count, offset and index is 64-bit.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

// Records per chunk.  One chunk is one 64-bit count and one trip through the scan: at 2 048 records (32 KiB) that is 8
// bytes per 32 KiB read, and a 4.5 * 10^7-record list is 22 000 chunks — a scan of 176 KB.  A workgroup of kCutThreads = 256
// threads holds a chunk as 8 records per lane, 32 VGPRs, all 8 loads in flight before the first is used; 8 such workgroups
// fill the 32 wave slots of a CU.  A smaller chunk leaves fewer loads in flight per lane, a larger one leaves a C2-sized
// list (4.5 * 10^5 records: 220 chunks) with fewer chunks than the device has CUs.
constexpr u32 kCutChunkEdges = KSP_CUT_CHUNK_EDGES;
constexpr int kCutThreads = 256;
constexpr int kCutWaves = kCutThreads / 64;
constexpr int kCutIters = (int)(kCutChunkEdges / kCutThreads);   // ballots per wave and chunk = records per lane
static_assert(kCutChunkEdges % kCutThreads == 0 && kCutIters * kCutThreads == (int)kCutChunkEdges, "a chunk is whole ballots of every wave");

// first record of wave `wave` in chunk `chunk` (a multiple of 64: a ballot never straddles two words of the ballot array)
__device__ inline u64 cut_wave_base(const u64 chunk, const u32 wave) { return chunk * kCutChunkEdges + (u64)wave * (kCutIters * 64); }

// a value every lane of the wave holds alike, moved to scalar registers (a ballot read back from memory)
__device__ inline unsigned long long cut_wave_uniform(const unsigned long long v) {
    const u32 lo = (u32)__builtin_amdgcn_readfirstlane((int)(u32)v), hi = (u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

template <bool kBallots>
__global__ __launch_bounds__(kCutThreads) void k_cut_count(const ksp_edge* __restrict__ ed, const u64 n, const u64 n_chunks, const u32* __restrict__ cnt,
                                                           const int col, const float vcrit, const int mode, u64* __restrict__ chunk_count,
                                                           unsigned long long* __restrict__ ballots) {
    __shared__ u32 wave_kept[kCutWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = cut_wave_base(chunk, wave);
        ksp_edge x[kCutIters];
#pragma unroll
        for (int k = 0; k < kCutIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            if (e < n) x[k] = ed[e];
        }
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kCutIters; ++k) {
            const u64 e = base + (u64)k * 64 + lane;
            const bool keep = e < n && cc_edge_kept(x[k], cnt, col, vcrit, mode);
            const unsigned long long b = __ballot(keep);
            kept += (u32)__popcll(b);
            if (kBallots && lane == 0 && e < n) ballots[e >> 6] = b;
        }
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 sum = 0;
            for (int w = 0; w < kCutWaves; ++w) sum += wave_kept[w];
            chunk_count[chunk] = sum;
        }
        __syncthreads();   // (wave_kept is written again for the next chunk)
    }
}

template <bool kBallots>
__global__ __launch_bounds__(kCutThreads) void k_cut_scatter(const ksp_edge* __restrict__ ed, const u64 n, const u64 n_chunks, const u32* __restrict__ cnt,
                                                             const int col, const float vcrit, const int mode, const u64* __restrict__ chunk_off,
                                                             const unsigned long long* __restrict__ ballots, ksp_edge* __restrict__ out) {
    __shared__ u32 wave_kept[kCutWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1;   // the lanes before mine
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 base = cut_wave_base(chunk, wave);
        ksp_edge x[kCutIters];
        unsigned long long b[kCutIters];
        if (kBallots) {
#pragma unroll
            for (int k = 0; k < kCutIters; ++k) {
                const u64 first = base + (u64)k * 64;
                b[k] = cut_wave_uniform(first < n ? ballots[first >> 6] : 0ull);
            }
#pragma unroll
            for (int k = 0; k < kCutIters; ++k)
                if ((b[k] >> lane) & 1) x[k] = ed[base + (u64)k * 64 + lane];   // (a set bit is a record below n)
                else x[k] = ksp_edge{0, 0, 0};
        } else {
#pragma unroll
            for (int k = 0; k < kCutIters; ++k) {
                const u64 e = base + (u64)k * 64 + lane;
                if (e < n) x[k] = ed[e];
            }
#pragma unroll
            for (int k = 0; k < kCutIters; ++k) {
                const u64 e = base + (u64)k * 64 + lane;
                b[k] = __ballot(e < n && cc_edge_kept(x[k], cnt, col, vcrit, mode));
            }
        }
        u32 kept = 0;
#pragma unroll
        for (int k = 0; k < kCutIters; ++k) kept += (u32)__popcll(b[k]);
        if (lane == 0) wave_kept[wave] = kept;
        __syncthreads();
        u64 pos = chunk_off[chunk];
        for (u32 w = 0; w < wave; ++w) pos += wave_kept[w];
        __syncthreads();   // (wave_kept is written again for the next chunk)
#pragma unroll
        for (int k = 0; k < kCutIters; ++k) {
            if ((b[k] >> lane) & 1) out[pos + (u64)__popcll(b[k] & below)] = x[k];
            pos += (u64)__popcll(b[k]);
        }
    }
}

// workgroups of both passes: one per chunk up to 8 per CU (32 waves: a full CU), the rest by the chunk loop.  (No list of 0
// chunks gets here — every caller has returned or refused n_edges == 0 before — so the at-least-1 of grid_of changes no launch.)
int cut_grid(const u64 n_chunks, unsigned* grid) {
    ksp::WorkgroupCap g;
    if (const int rc = ksp::workgroup_cap("KSP_CUT_MAX_WORKGROUPS", "cut", g)) return rc;
    *grid = g.grid_of(n_chunks);
    return KSP_OK;
}

// the scatter pass reads the count pass's ballots unless KSP_CUT_BALLOTS=0 (evaluate the predicate again)
bool cut_keep_ballots() {
    const char* kb = std::getenv("KSP_CUT_BALLOTS");
    return !(kb && std::strcmp(kb, "0") == 0);
}

struct CutKeptFn {   // the same predicate as a functor: the library yardstick of ksp_debug_cut_times
    const u32* cnt;
    int col;
    float vcrit;
    int mode;
    __device__ bool operator()(const ksp_edge& x) const { return cc_edge_kept(x, cnt, col, vcrit, mode); }
};

int check_cut_args(const char* who, const ksp_edge* d_edges, const u64 n_edges, const u32* d_kmer_counts, const int dist_col, const double cutoff,
                   const ksp_edge* d_out) {
    if (n_edges && (!d_edges || !d_kmer_counts || !d_out)) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { ksp::set_error(std::string(who) + ": dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (cutoff != cutoff) { ksp::set_error(std::string(who) + ": the cut-off is NaN"); return KSP_E_ARG; }
    if (n_edges) {
        const uintptr_t a = (uintptr_t)d_edges, b = (uintptr_t)d_out;
        const u64 span = n_edges > (~0ull) / sizeof(ksp_edge) ? ~0ull : n_edges * sizeof(ksp_edge);
        if ((a <= b ? b - a : a - b) < span) { ksp::set_error(std::string(who) + ": d_out overlaps d_edges"); return KSP_E_ARG; }
    }
    return KSP_OK;
}

}  // namespace

namespace ksp {
void CutPass::release() {
    if (d_off) (void)hipFree(d_off);
    if (d_ballots) (void)hipFree(d_ballots);
    d_off = nullptr;
    d_ballots = nullptr;
    n_chunks = 0;
}

// count + scan over n_edges > 0 records on the CURRENT device; the pass keeps what the scatter needs
int cut_count_on_device(const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, const double cutoff, CutPass& pass,
                        uint64_t* n_kept) {
    int rc = KSP_OK;
    DeviceArena A;   // (the pass outlives this call: its two arrays are its own)
    u64* d_count = nullptr;
    void* d_tmp = nullptr;
    size_t tb = 0;
    unsigned grid = 1;
    unsigned long long total = 0;
    *n_kept = 0;
    pass.release();
    if (n_edges == 0) return KSP_OK;
    cc_critical(cutoff, &pass.vcrit, &pass.mode);
    pass.n_chunks = (n_edges + kCutChunkEdges - 1) / kCutChunkEdges;
    if ((rc = cut_grid(pass.n_chunks, &grid))) return rc;
    if ((rc = A.alloc(&d_count, (size_t)(pass.n_chunks + 1)))) goto done;
    KSP_TRY_HIP(hipMalloc((void**)&pass.d_off, (size_t)(pass.n_chunks + 1) * 8));
    KSP_TRY_HIP(hipMemsetAsync(d_count + pass.n_chunks, 0, 8, nullptr));   // (the scan's last output is then the total)
    if (cut_keep_ballots()) {
        KSP_TRY_HIP(hipMalloc((void**)&pass.d_ballots, (size_t)((n_edges + 63) / 64) * 8));
        hipLaunchKernelGGL(k_cut_count<true>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, pass.n_chunks, d_cnt, col, pass.vcrit, pass.mode,
                           d_count, pass.d_ballots);
    } else {
        hipLaunchKernelGGL(k_cut_count<false>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, pass.n_chunks, d_cnt, col, pass.vcrit, pass.mode,
                           d_count, (unsigned long long*)nullptr);
    }
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb, d_count, pass.d_off, (u64)0, (size_t)(pass.n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    if ((rc = A.alloc_bytes(&d_tmp, tb ? tb : 8))) goto done;
    KSP_TRY_HIP(rocprim::exclusive_scan(d_tmp, tb, d_count, pass.d_off, (u64)0, (size_t)(pass.n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    KSP_TRY_HIP(hipMemcpy(&total, pass.d_off + pass.n_chunks, 8, hipMemcpyDeviceToHost));
    *n_kept = total;
done:
    if (rc) pass.release();
    return rc;
}

// the kept records of the counted list into d_out (room for the count pass's total), in their input order
int cut_scatter_on_device(const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const int col, const CutPass& pass, ksp_edge* d_out) {
    int rc = KSP_OK;
    unsigned grid = 1;
    if (n_edges == 0 || pass.n_chunks == 0) return KSP_OK;
    if ((rc = cut_grid(pass.n_chunks, &grid))) return rc;
    if (pass.d_ballots)
        hipLaunchKernelGGL(k_cut_scatter<true>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, pass.n_chunks, d_cnt, col, pass.vcrit, pass.mode,
                           pass.d_off, pass.d_ballots, d_out);
    else
        hipLaunchKernelGGL(k_cut_scatter<false>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, pass.n_chunks, d_cnt, col, pass.vcrit, pass.mode,
                           pass.d_off, (const unsigned long long*)nullptr, d_out);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(hipDeviceSynchronize());
done:
    return rc;
}
}  // namespace ksp

extern "C" int ksp_edges_cut(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, double cutoff,
                             ksp_edge* d_out, uint64_t* n_kept) {
    if (!n_kept) { ksp::set_error("ksp_edges_cut: NULL argument"); return KSP_E_ARG; }
    if (const int rc = check_cut_args("ksp_edges_cut", d_edges, n_edges, d_kmer_counts, dist_col, cutoff, d_out)) return rc;
    if (const int rc = ksp::set_device("ksp_edges_cut", device)) return rc;
    *n_kept = 0;
    if (n_edges == 0) return KSP_OK;   // no kernel runs
    ksp::CutPass pass;
    int rc = ksp::cut_count_on_device(d_edges, n_edges, d_kmer_counts, dist_col, cutoff, pass, n_kept);
    if (!rc && *n_kept) rc = ksp::cut_scatter_on_device(d_edges, n_edges, d_kmer_counts, dist_col, pass, d_out);
    pass.release();
    return rc;
}

// (tools/cut_times.py) HIP-event times of `reps` runs of one way to cut the same list: which 0 = count + scan + scatter with
// the predicate evaluated twice, 1 = with the count pass's ballots, 2 = rocprim::select with the same predicate as a functor.
// Each time covers the kernels, the scan and the 8-byte read of the total; allocations are outside.  ms[reps].
extern "C" int ksp_debug_cut_times(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, double cutoff,
                                   ksp_edge* d_out, int which, int reps, float* ms, uint64_t* n_kept) {
    if (!n_kept || !ms || reps < 1 || which < 0 || which > 2 || n_edges == 0) { ksp::set_error("ksp_debug_cut_times: bad argument"); return KSP_E_ARG; }
    if (const int rc = check_cut_args("ksp_debug_cut_times", d_edges, n_edges, d_kmer_counts, dist_col, cutoff, d_out)) return rc;
    if (const int rc = ksp::set_device("ksp_debug_cut_times", device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    float vcrit = 0;
    int mode = 0;
    ksp::cc_critical(cutoff, &vcrit, &mode);
    const u64 n_chunks = (n_edges + kCutChunkEdges - 1) / kCutChunkEdges;
    u64 *d_count = nullptr, *d_off = nullptr;
    unsigned long long *d_ballots = nullptr, *d_nsel = nullptr;
    void* d_tmp = nullptr;
    size_t tb_scan = 0, tb_sel = 0;
    unsigned grid = 1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    const CutKeptFn fn{d_kmer_counts, dist_col, vcrit, mode};
    if ((rc = cut_grid(n_chunks, &grid))) return rc;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    if ((rc = A.alloc(&d_count, (size_t)(n_chunks + 1))) || (rc = A.alloc(&d_off, (size_t)(n_chunks + 1))) ||
        (rc = A.alloc(&d_ballots, (size_t)((n_edges + 63) / 64))) || (rc = A.alloc(&d_nsel, 1)))
        goto done;
    KSP_TRY_HIP(hipMemset(d_count + n_chunks, 0, 8));
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, d_count, d_off, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    KSP_TRY_HIP(rocprim::select(nullptr, tb_sel, d_edges, d_out, d_nsel, (size_t)n_edges, fn, (hipStream_t) nullptr));
    if ((rc = A.alloc_bytes(&d_tmp, std::max<size_t>(std::max(tb_scan, tb_sel), 8)))) goto done;
    for (int r = 0; r < reps; ++r) {
        unsigned long long total = 0;
        KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
        if (which == 2) {
            KSP_TRY_HIP(rocprim::select(d_tmp, tb_sel, d_edges, d_out, d_nsel, (size_t)n_edges, fn, (hipStream_t) nullptr));
            KSP_TRY_HIP(hipMemcpy(&total, d_nsel, 8, hipMemcpyDeviceToHost));
        } else {
            if (which == 1)
                hipLaunchKernelGGL(k_cut_count<true>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_kmer_counts, dist_col, vcrit, mode, d_count, d_ballots);
            else
                hipLaunchKernelGGL(k_cut_count<false>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_kmer_counts, dist_col, vcrit, mode, d_count,
                                   (unsigned long long*)nullptr);
            KSP_TRY_HIP(rocprim::exclusive_scan(d_tmp, tb_scan, d_count, d_off, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
            KSP_TRY_HIP(hipMemcpy(&total, d_off + n_chunks, 8, hipMemcpyDeviceToHost));
            if (which == 1)
                hipLaunchKernelGGL(k_cut_scatter<true>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_kmer_counts, dist_col, vcrit, mode, d_off,
                                   d_ballots, d_out);
            else
                hipLaunchKernelGGL(k_cut_scatter<false>, dim3(grid), dim3(kCutThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_kmer_counts, dist_col, vcrit, mode, d_off,
                                   (const unsigned long long*)nullptr, d_out);
            KSP_TRY_HIP(hipGetLastError());
        }
        KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
        KSP_TRY_HIP(hipEventSynchronize(ev1));
        KSP_TRY_HIP(hipEventElapsedTime(&ms[r], ev0, ev1));
        *n_kept = total;
    }
done:
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}
