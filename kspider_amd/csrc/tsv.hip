// The rows of the pairwise TSV as text, made on the device from the join's ksp_edge records:
//     id1 \t id2 \t shared \t min \t avg \t max \n
// byte for byte what index_io.cpp::format_rows prints for the same record.  The digits of the three floats come from the
// integer formulation of tsv_text.h; no floating-point operation takes part in a digit.
//
// Rows are processed in chunks of KSP_TSV_CHUNK_ROWS = 256, one row per lane of a 256-thread workgroup, one chunk per pass of
// a workgroup's chunk loop.  Three passes, ordered by kernel boundaries alone:
//   count   every lane finds its row's fields and digits and counts the bytes of its text; the workgroup adds them up: one
//           64-bit byte count per chunk.  A row that cannot be printed raises the flag (an ordinary store).
//   scan    exclusive scan of the chunk counts (rocPRIM): every chunk's 64-bit base and, behind the last chunk, the total
//   write   the same chunks again: a scan of the row lengths over the workgroup places every row in LDS, each lane writes its
//           row's text there once, and the chunk goes to global memory.  A chunk's base is an arbitrary byte address, so the
//           text is staged at the base's offset modulo 16: the copy out is aligned 16-byte stores, with byte stores only in
//           the first and last 16 bytes of the chunk.
// The digits are found twice (count, write); what is never made is a row-by-82-bytes scratch in HBM.  The text leaves the
// device through a window of whole chunks in HBM and from there in pieces through two pinned staging buffers, so neither the
// device nor the host holds more than a window of it: 4.5 * 10^7 rows are about 2 GB of text.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "edge_cut.hip.h"
#include "engine_internal.h"
#include "index_io.h"
#include "tsv_text.h"

typedef uint32_t u32;
typedef uint64_t u64;

namespace {

constexpr u32 kTsvChunkRows = KSP_TSV_CHUNK_ROWS;
constexpr int kTsvThreads = 256;
constexpr int kTsvWaves = kTsvThreads / 64;
static_assert(kTsvChunkRows == (u32)kTsvThreads, "one row per lane");
// LDS of the write pass: the longest chunk behind the largest staging offset, in whole 16-byte vectors (20 240 bytes: seven
// workgroups of a CU's 160 KiB, 28 of its 32 wave slots)
constexpr u32 kTsvLdsBytes = (15 + kTsvChunkRows * KSP_TSV_ROW_MAX + 15) / 16 * 16;
constexpr u64 kTsvPieceDefault = 8ull << 20;   // bytes per pinned staging buffer; the window in HBM is 8 pieces (unmeasured choices)

// the fields and digits of record x, or false: an end that is no node, or a column outside the domain of tsv_text.h (NaN too)
__device__ inline bool tsv_row(const ksp_edge& x, const u32* __restrict__ cnt, const u32* __restrict__ ids, const u32 n_nodes, ksp_tsv::RowText& r) {
    if (x.source_1 >= n_nodes || x.source_2 >= n_nodes) return false;
    float mn, av, mx;
    edge_col_values(x, cnt, &mn, &av, &mx);
    r.id1 = ids ? ids[x.source_1] : x.source_1;
    r.id2 = ids ? ids[x.source_2] : x.source_2;
    r.shared = x.shared;
    r.col[0] = ksp_tsv::float_digits(__float_as_uint(mn));
    r.col[1] = ksp_tsv::float_digits(__float_as_uint(av));
    r.col[2] = ksp_tsv::float_digits(__float_as_uint(mx));
    return r.col[0].kind != ksp_tsv::FloatDigits::kRefused && r.col[1].kind != ksp_tsv::FloatDigits::kRefused &&
           r.col[2].kind != ksp_tsv::FloatDigits::kRefused;
}

// inclusive scan over the 64 lanes of a wave
__device__ inline u32 tsv_wave_scan(u32 v, const u32 lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 t = (u32)__shfl_up((int)v, d, 64);
        if (lane >= (u32)d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(kTsvThreads) void k_tsv_count(const ksp_edge* __restrict__ ed, const u64 n, const u64 n_chunks, const u32* __restrict__ cnt,
                                                           const u32* __restrict__ ids, const u32 n_nodes, u64* __restrict__ chunk_bytes,
                                                           u32* __restrict__ flag) {
    __shared__ u32 wave_sum[kTsvWaves];
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const u64 i = chunk * kTsvChunkRows + threadIdx.x;
        u32 len = 0;
        if (i < n) {
            ksp_tsv::RowText r;
            if (tsv_row(ed[i], cnt, ids, n_nodes, r)) {
                ksp_tsv::Counter c;
                ksp_tsv::emit_row(c, r);
                len = c.n;
            } else {
                *flag = 1;
            }
        }
        const u32 incl = tsv_wave_scan(len, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        if (threadIdx.x == 0) {
            u64 sum = 0;
            for (int w = 0; w < kTsvWaves; ++w) sum += wave_sum[w];
            chunk_bytes[chunk] = sum;
        }
        __syncthreads();   // (wave_sum is written again for the next chunk)
    }
}

// chunks [c0, c1) into the window: byte `b` of the text goes to win[b - win_base]; win and win_base are multiples of 16
__global__ __launch_bounds__(kTsvThreads) void k_tsv_write(const ksp_edge* __restrict__ ed, const u64 n, const u64 c0, const u64 c1, const u32* __restrict__ cnt,
                                                           const u32* __restrict__ ids, const u32 n_nodes, const u64* __restrict__ chunk_off,
                                                           const u64 win_base, char* __restrict__ win) {
    __shared__ uint4 text4[kTsvLdsBytes / 16];
    __shared__ u32 wave_sum[kTsvWaves];
    char* const text = (char*)text4;
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 chunk = c0 + blockIdx.x; chunk < c1; chunk += gridDim.x) {
        const u64 i = chunk * kTsvChunkRows + threadIdx.x;
        u32 len = 0;
        ksp_tsv::RowText r;
        if (i < n && tsv_row(ed[i], cnt, ids, n_nodes, r)) {
            ksp_tsv::Counter c;
            ksp_tsv::emit_row(c, r);
            len = c.n;
        }
        const u32 incl = tsv_wave_scan(len, lane);
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        u32 before = 0, total = 0;
        for (u32 w = 0; w < (u32)kTsvWaves; ++w) {
            if (w < wave) before += wave_sum[w];
            total += wave_sum[w];
        }
        const u64 base = chunk_off[chunk];
        const u32 s = (u32)(base & 15);   // the staging offset: LDS byte j is text byte base - s + j
        if (len && s + before + incl <= kTsvLdsBytes) {   // (always: a row is at most KSP_TSV_ROW_MAX bytes)
            ksp_tsv::Writer w{text + s + before + incl - len};
            ksp_tsv::emit_row(w, r);
        }
        __syncthreads();
        char* const g = win + (base - s - win_base);
        const u32 end = s + total;
        for (u32 k = threadIdx.x; k * 16 < end && k < kTsvLdsBytes / 16; k += kTsvThreads) {
            const u32 lo = k * 16, hi = lo + 16;
            if (lo >= s && hi <= end) ((uint4*)g)[k] = text4[k];
            else
                for (u32 j = lo < s ? s : lo; j < (hi < end ? hi : end); ++j) g[j] = text[j];
        }
        __syncthreads();   // (text and wave_sum are written again for the next chunk)
    }
}

// (ksp_debug_format_floats) the text of value i into text[16 * i ...], its length into len[i]; a value outside the domain: the flag
__global__ void k_tsv_floats(const u32* __restrict__ bits, const u64 n, char* __restrict__ text, u32* __restrict__ len, u32* __restrict__ flag) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const ksp_tsv::FloatDigits f = ksp_tsv::float_digits(bits[i]);
        if (f.kind == ksp_tsv::FloatDigits::kRefused) { *flag = 1; len[i] = 0; continue; }
        ksp_tsv::Counter c;
        ksp_tsv::emit_float(c, f);
        ksp_tsv::Writer w{text + 16 * i};
        if (c.n <= KSP_TSV_FLOAT_MAX) ksp_tsv::emit_float(w, f);
        len[i] = c.n;
    }
}

// (ksp_debug_tsv_records) seeded inputs of the timing tool, made where they are read
__device__ inline u64 tsv_mix(u64 x) {   // splitmix64's finalizer
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ inline u32 tsv_fill_count(const u64 seed, const u32 v) { return 1000u + (u32)(tsv_mix(seed ^ v) % 999001u); }   // 10^3 .. 10^6
__global__ void k_tsv_fill_nodes(const u64 seed, const u32 n_nodes, u32* __restrict__ cnt, u32* __restrict__ ids) {
    for (u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += (u64)gridDim.x * blockDim.x) {
        cnt[v] = tsv_fill_count(seed, (u32)v);
        ids[v] = (u32)v + 1;
    }
}
__global__ void k_tsv_fill_edges(const u64 seed, const u32 n_nodes, const u64 n, ksp_edge* __restrict__ ed) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 a = (u32)((unsigned __int128)i * (n_nodes - 1) / n);                                  // ascending, below n_nodes - 1
        const u32 b = a + 1 + (u32)(tsv_mix(seed + 2 * i) % (n_nodes - 1 - a));                       // a < b < n_nodes
        const u32 smaller = min(tsv_fill_count(seed, a), tsv_fill_count(seed, b));
        ed[i] = ksp_edge{a, b, 1 + tsv_mix(seed + 2 * i + 1) % smaller};                                // 1 .. the smaller count
    }
}

int tsv_grid(const u64 n_chunks, unsigned* grid) {
    ksp::WorkgroupCap g;
    if (const int rc = ksp::workgroup_cap("KSP_TSV_MAX_WORKGROUPS", "ksp_edges_tsv", g)) return rc;
    *grid = g.grid_of(n_chunks);
    return KSP_OK;
}

u64 tsv_piece_bytes() {
    const char* pv = std::getenv("KSP_TSV_PIECE");
    const long long v = pv ? std::atoll(pv) : 0;
    return v >= 1 ? (u64)v : kTsvPieceDefault;
}

struct HostPinned {   // pinned host memory of one call
    void* p = nullptr;
    ~HostPinned() { if (p) (void)hipHostFree(p); }
};

// the two passes' device time, by HIP events (ksp_debug_tsv_times), when asked for
struct KernelClock {
    float* ms = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~KernelClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    int init(float* out) {
        ms = out;
        if (!ms) return KSP_OK;
        *ms = 0;
        KSP_HIP(hipEventCreate(&e0));
        KSP_HIP(hipEventCreate(&e1));
        return KSP_OK;
    }
    int start() { if (ms) KSP_HIP(hipEventRecord(e0, nullptr)); return KSP_OK; }
    int stop() {
        if (!ms) return KSP_OK;
        float t = 0;
        KSP_HIP(hipEventRecord(e1, nullptr));
        KSP_HIP(hipEventSynchronize(e1));
        KSP_HIP(hipEventElapsedTime(&t, e0, e1));
        *ms += t;
        return KSP_OK;
    }
};

const char* const kTsvRefused = ": a row names a source >= n_nodes or has a column that has no text here (a NaN, or a value outside [2^-40, 2^40))";

}  // namespace

namespace ksp {

// ksp_edges_tsv on the CURRENT device.  sink == nullptr: only *n_bytes (the size query).  Otherwise the text is handed to sink
// in order, in pieces of at most $KSP_TSV_PIECE bytes that live in pinned memory until sink returns; a sink that returns a code
// other than KSP_OK (with its text in ksp_last_error()) ends the call with it.  capacity < *n_bytes: KSP_E_OVERFLOW, sink is
// never called.  ms_kernels (may be NULL): the device time of the count, scan and write passes.
int tsv_edges_on_device(const char* who, const uint32_t n_nodes, const ksp_edge* d_edges, const uint64_t n_edges, const uint32_t* d_cnt, const uint32_t* d_ids,
                        const uint64_t capacity, const TsvSink* sink, uint64_t* n_bytes, float* ms_kernels) {
    int rc = KSP_OK;
    DeviceArena A;
    HostPinned pin[2];
    KernelClock clock;
    hipStream_t cs = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    u64 *d_count = nullptr, *d_off = nullptr;
    u32* d_flag = nullptr;
    char* d_win = nullptr;
    void* d_tmp = nullptr;
    size_t tb = 0;
    unsigned grid = 1;
    u32 flag = 0;
    std::vector<u64> off;
    *n_bytes = 0;
    if (n_edges == 0) return KSP_OK;   // no kernel runs
    const u64 n_chunks = (n_edges + kTsvChunkRows - 1) / kTsvChunkRows;
    const u64 piece = tsv_piece_bytes();
    const u64 window = std::max<u64>((std::min<u64>(piece, 1ull << 40) * 8 + 15) / 16 * 16, kTsvLdsBytes);   // holds the longest chunk at any staging offset
    if ((rc = clock.init(ms_kernels)) || (rc = tsv_grid(n_chunks, &grid))) return rc;
    if ((rc = device_fits(who, (n_chunks + 1) * 16 + 64, "the chunk counts and offsets"))) return rc;
    if ((rc = A.alloc(&d_count, (size_t)(n_chunks + 1))) || (rc = A.alloc(&d_off, (size_t)(n_chunks + 1))) || (rc = A.alloc(&d_flag, 1))) return rc;
    KSP_TRY_HIP(hipMemsetAsync(d_count + n_chunks, 0, 8, nullptr));   // (the scan's last output is then the total)
    KSP_TRY_HIP(hipMemsetAsync(d_flag, 0, 4, nullptr));
    KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb, d_count, d_off, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    if ((rc = A.alloc_bytes(&d_tmp, tb ? tb : 8))) return rc;
    if ((rc = clock.start())) return rc;
    hipLaunchKernelGGL(k_tsv_count, dim3(grid), dim3(kTsvThreads), 0, nullptr, d_edges, n_edges, n_chunks, d_cnt, d_ids, n_nodes, d_count, d_flag);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(rocprim::exclusive_scan(d_tmp, tb, d_count, d_off, (u64)0, (size_t)(n_chunks + 1), rocprim::plus<u64>(), (hipStream_t) nullptr));
    if ((rc = clock.stop())) return rc;
    KSP_TRY_HIP(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
    if (flag) { set_error(std::string(who) + kTsvRefused); return KSP_E_ARG; }
    off.resize((size_t)n_chunks + 1);
    KSP_TRY_HIP(hipMemcpy(off.data(), d_off, (size_t)(n_chunks + 1) * 8, hipMemcpyDeviceToHost));
    *n_bytes = off[(size_t)n_chunks];
    if (!sink) return KSP_OK;
    if (capacity < *n_bytes) { set_error(std::string(who) + ": the text is " + std::to_string(*n_bytes) + " bytes, the buffer holds " + std::to_string(capacity)); return KSP_E_OVERFLOW; }
    if ((rc = device_fits(who, window, "the text window"))) return rc;
    if ((rc = A.alloc(&d_win, (size_t)window))) return rc;
    KSP_TRY_HIP(hipHostMalloc(&pin[0].p, (size_t)piece));
    KSP_TRY_HIP(hipHostMalloc(&pin[1].p, (size_t)piece));
    KSP_TRY_HIP(hipStreamCreate(&cs));
    KSP_TRY_HIP(hipEventCreate(&ev[0]));
    KSP_TRY_HIP(hipEventCreate(&ev[1]));
    for (u64 c0 = 0; c0 < n_chunks;) {
        // the window: as many whole chunks as fit behind the 16-byte boundary below the first one's base
        const u64 win_base = off[(size_t)c0] & ~15ull;
        u64 c1 = c0 + 1;   // (one chunk always fits: window >= kTsvLdsBytes)
        while (c1 < n_chunks && off[(size_t)c1 + 1] - win_base <= window) ++c1;
        if (off[(size_t)c1] - win_base > window) { set_error(std::string(who) + ": a chunk of text longer than its bound"); rc = KSP_E_HIP; goto done; }
        if ((rc = clock.start())) goto done;
        hipLaunchKernelGGL(k_tsv_write, dim3(std::min<u64>(grid, c1 - c0)), dim3(kTsvThreads), 0, nullptr, d_edges, n_edges, c0, c1, d_cnt, d_ids, n_nodes, d_off,
                           win_base, d_win);
        KSP_TRY_HIP(hipGetLastError());
        if ((rc = clock.stop())) goto done;
        KSP_TRY_HIP(hipStreamSynchronize(nullptr));
        // out in pieces: while the host takes piece k - 1 from one staging buffer, piece k is copied into the other
        const u64 t0 = off[(size_t)c0], t1 = off[(size_t)c1];
        u64 prev_len = 0;
        int prev = -1, cur = 0;
        for (u64 t = t0; t < t1; t += piece, cur ^= 1) {
            const u64 len = std::min<u64>(piece, t1 - t);
            KSP_TRY_HIP(hipMemcpyAsync(pin[cur].p, d_win + (t - win_base), (size_t)len, hipMemcpyDeviceToHost, cs));
            KSP_TRY_HIP(hipEventRecord(ev[cur], cs));
            if (prev >= 0) {
                KSP_TRY_HIP(hipEventSynchronize(ev[prev]));
                if ((rc = (*sink)((const char*)pin[prev].p, prev_len))) goto done;
            }
            prev = cur;
            prev_len = len;
        }
        if (prev >= 0) {   // (the window is free again once its last piece has left it)
            KSP_TRY_HIP(hipEventSynchronize(ev[prev]));
            if ((rc = (*sink)((const char*)pin[prev].p, prev_len))) goto done;
        }
        c0 = c1;
    }
done:
    if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    return rc;
}

}  // namespace ksp

extern "C" int ksp_edges_tsv(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, const uint32_t* d_ids,
                             char* h_text, uint64_t capacity, uint64_t* n_bytes) {
    if (!n_bytes || !d_kmer_counts || (n_edges && !d_edges)) { ksp::set_error("ksp_edges_tsv: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_edges_tsv", device)) return rc;
    u64 pos = 0;
    const ksp::TsvSink sink = [&](const char* p, const uint64_t n) {
        std::memcpy(h_text + pos, p, (size_t)n);
        pos += n;
        return (int)KSP_OK;
    };
    return ksp::tsv_edges_on_device("ksp_edges_tsv", n_nodes, d_edges, n_edges, d_kmer_counts, d_ids, capacity, h_text ? &sink : nullptr, n_bytes, nullptr);
}

// (tests) the device formatter of tsv_text.h on n host floats: h_text[16 * i ...] holds the h_len[i] bytes of value i's text
extern "C" int ksp_debug_format_floats(int device, const float* h_values, uint64_t n, char* h_text, uint32_t* h_len) {
    if (n && (!h_values || !h_text || !h_len)) { ksp::set_error("ksp_debug_format_floats: NULL argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_debug_format_floats", device)) return rc;
    if (n == 0) return KSP_OK;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    u32 *d_bits = nullptr, *d_len = nullptr, *d_flag = nullptr;
    char* d_text = nullptr;
    u32 flag = 0;
    if ((rc = ksp::device_fits("ksp_debug_format_floats", n * 24 + 64, "")) || (rc = A.alloc(&d_bits, (size_t)n)) || (rc = A.alloc(&d_len, (size_t)n)) ||
        (rc = A.alloc(&d_flag, 1)) || (rc = A.alloc(&d_text, (size_t)n * 16)))
        return rc;
    KSP_TRY_HIP(hipMemcpy(d_bits, h_values, (size_t)n * 4, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemset(d_flag, 0, 4));
    KSP_TRY_HIP(hipMemset(d_text, 0, (size_t)n * 16));
    hipLaunchKernelGGL(k_tsv_floats, dim3((unsigned)std::min<u64>((n + 255) / 256, 1u << 16)), dim3(256), 0, nullptr, d_bits, n, d_text, d_len, d_flag);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(hipMemcpy(&flag, d_flag, 4, hipMemcpyDeviceToHost));
    if (flag) { ksp::set_error("ksp_debug_format_floats: a value outside the domain (0, +inf, [2^-40, 2^40))"); return KSP_E_ARG; }
    KSP_TRY_HIP(hipMemcpy(h_text, d_text, (size_t)n * 16, hipMemcpyDeviceToHost));
    KSP_TRY_HIP(hipMemcpy(h_len, d_len, (size_t)n * 4, hipMemcpyDeviceToHost));
done:
    return rc;
}

// (tools/tsv_times.py) valid seeded inputs made on the device: n_nodes >= 2 sources with ids index + 1 and k-mer counts of 10^3 .. 10^6,
// n_edges records with source_1 ascending, source_1 < source_2 and a shared count between 1 and the smaller of the two counts
extern "C" int ksp_debug_tsv_records(int device, uint32_t n_nodes, uint64_t n_edges, uint64_t seed, ksp_edge* d_edges, uint32_t* d_kmer_counts, uint32_t* d_ids) {
    if (n_nodes < 2 || !d_kmer_counts || !d_ids || (n_edges && !d_edges)) { ksp::set_error("ksp_debug_tsv_records: bad argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_debug_tsv_records", device)) return rc;
    int rc = KSP_OK;
    hipLaunchKernelGGL(k_tsv_fill_nodes, dim3((n_nodes + 255) / 256), dim3(256), 0, nullptr, seed, n_nodes, d_kmer_counts, d_ids);
    if (n_edges) hipLaunchKernelGGL(k_tsv_fill_edges, dim3((unsigned)std::min<u64>((n_edges + 255) / 256, 1u << 16)), dim3(256), 0, nullptr, seed, n_nodes, n_edges, d_edges);
    KSP_TRY_HIP(hipGetLastError());
    KSP_TRY_HIP(hipDeviceSynchronize());
done:
    return rc;
}

// (tools/tsv_times.py) `reps` runs of one way to turn the same records into row text in host memory; no file is written.
//   which 0: the device's text kernels and the copy of the text to pinned host memory (ksp_edges_tsv without its last memcpy)
//   which 1: the copy of the records to pinned host memory, then index_io.cpp's format_rows with `threads` host threads
// ms[2 * r] = wall time of run r in ms; ms[2 * r + 1] = which 0: the kernels' own time by HIP events, which 1: the copy's time.
extern "C" int ksp_debug_tsv_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, const uint32_t* d_ids,
                                   int which, int reps, int threads, float* ms) {
    typedef std::chrono::steady_clock Clock;
    if (!ms || reps < 1 || which < 0 || which > 1 || threads < 1 || n_edges == 0 || !d_edges || !d_kmer_counts) { ksp::set_error("ksp_debug_tsv_times: bad argument"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device("ksp_debug_tsv_times", device)) return rc;
    int rc = KSP_OK;
    if (which == 0) {
        for (int r = 0; r < reps && !rc; ++r) {
            u64 bytes = 0, got = 0;
            const ksp::TsvSink sink = [&](const char*, const uint64_t n) { got += n; return (int)KSP_OK; };
            const auto t0 = Clock::now();
            rc = ksp::tsv_edges_on_device("ksp_debug_tsv_times", n_nodes, d_edges, n_edges, d_kmer_counts, d_ids, ~0ull, &sink, &bytes, &ms[2 * r + 1]);
            ms[2 * r] = std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
            if (!rc && got != bytes) { ksp::set_error("ksp_debug_tsv_times: the pieces do not add up to the text"); rc = KSP_E_HIP; }
        }
        return rc;
    }
    // the host writer's inputs, outside the timed region: the id and the k-mer count of every node, as run_job holds them
    std::vector<u32> ids(n_nodes), counts(n_nodes);
    std::unordered_map<u32, u32> kmer_count;
    HostPinned pinned;
    KSP_TRY_HIP(hipMemcpy(counts.data(), d_kmer_counts, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    if (d_ids) KSP_TRY_HIP(hipMemcpy(ids.data(), d_ids, (size_t)n_nodes * 4, hipMemcpyDeviceToHost));
    else for (u32 v = 0; v < n_nodes; ++v) ids[v] = v;
    for (u32 v = 0; v < n_nodes; ++v) kmer_count[ids[v]] = counts[v];
    KSP_TRY_HIP(hipHostMalloc(&pinned.p, (size_t)n_edges * sizeof(ksp_edge)));
    for (int r = 0; r < reps; ++r) {
        const auto t0 = Clock::now();
        KSP_TRY_HIP(hipMemcpy(pinned.p, d_edges, (size_t)n_edges * sizeof(ksp_edge), hipMemcpyDeviceToHost));
        ms[2 * r + 1] = std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
        const ksp_edge* e = (const ksp_edge*)pinned.p;
        for (u64 i = 0; i < n_edges; ++i)
            if (e[i].source_1 >= n_nodes || e[i].source_2 >= n_nodes) { ksp::set_error("ksp_debug_tsv_times: a row names a source >= n_nodes"); return KSP_E_ARG; }
        std::vector<ksp::EdgeRow> rows;   // (merge_rows' share of the host path: the records as rows of ids)
        rows.reserve((size_t)n_edges);
        for (u64 i = 0; i < n_edges; ++i) rows.push_back(ksp::EdgeRow{ids[e[i].source_1], ids[e[i].source_2], e[i].shared});
        const size_t T = (size_t)std::min(threads, 64), chunk = 1 << 16;   // write_pairwise_tsv's loop without the file
        u64 total = 0;
        for (size_t base = 0; base < rows.size(); base += chunk * T) {
            std::vector<std::string> parts(T);
            std::vector<std::thread> th;
            for (size_t t = 0; t < T; ++t) {
                const size_t lo = std::min(rows.size(), base + t * chunk), hi = std::min(rows.size(), lo + chunk);
                if (lo >= hi) break;
                if (T == 1) ksp::format_rows(rows, lo, hi, kmer_count, parts[t]);
                else th.emplace_back(ksp::format_rows, std::cref(rows), lo, hi, std::cref(kmer_count), std::ref(parts[t]));
            }
            for (auto& x : th) x.join();
            for (auto& s : parts) total += s.size();
        }
        ms[2 * r] = std::chrono::duration<float, std::milli>(Clock::now() - t0).count();
        if (total == 0) { ksp::set_error("ksp_debug_tsv_times: no text"); return KSP_E_HIP; }
    }
done:
    return rc;
}
