// The device part of the sketcher: bytes of FASTA / FASTQ records in HBM -> sourmash-compatible FracMinHash
// sketches.  The arithmetic — codes, reverse complement, the k-mer's text, Murmur — is sketch_hash.h, for the protein, dayhoff
// and hp molecule types sketch_mol.h, both shared with the host loop.
//
//   hash     one pass over the bytes, sketch_kernels.hip.h: one tile frame and what k_sketch_hash (DNA), k_sketch_hash_protein
//            and k_sketch_hash_translated add to it.  It leaves the survivors, about 1 in `scaled`, as unsorted (hash, source)
//            records and counts them past the capacity without writing past it.
//   select   this file: rocPRIM's merge sort by (source, hash), one scan of head flags (an entry that differs from the one
//            before), k_sketch_compact writes the heads' hashes, k_sketch_offsets the per-source bounds by binary search.  The
//            counted calls launch k_sketch_compact_abund instead: a head also writes the length of its run, its
//            abundance.  The same for every molecule type.
// Every loop is bounded by a size the host computed; no workgroup waits on another; the result does not depend on scheduling.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"
#include "sketch_hash.h"
#include "sketch_mol.h"

namespace {

namespace sk = ksp_sketch;
typedef uint32_t u32;
typedef uint64_t u64;

#include "sketch_kernels.hip.h"

struct RecBefore {
    __host__ __device__ bool operator()(const Rec& a, const Rec& b) const { return a.src != b.src ? a.src < b.src : a.hash < b.hash; }
};

// 1 for a sorted entry that differs from the one before it, 0 behind the end
struct HeadFlag {
    const Rec* rec;
    u64 n;
    __host__ __device__ u64 operator()(const u64 i) const {
        if (i >= n) return 0;
        return i == 0 || rec[i].src != rec[i - 1].src || rec[i].hash != rec[i - 1].hash;
    }
};

inline auto head_flags_of(const Rec* rec, const u64 n) { return rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), HeadFlag{rec, n}); }

// scan[i] = heads before entry i (n + 1 values: the last is their number)
__global__ void k_sketch_compact(const Rec* __restrict__ rec, const u64* __restrict__ scan, const u64 n, u64* __restrict__ out_keys) {
    const HeadFlag head{rec, n};
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (head(i)) out_keys[scan[i]] = rec[i].hash;
}

// the same, and beside its hash a head writes the length of its run: the next head's index - its own, clamped at 2^32 - 1.  The next
// head is one before the first x > i whose scan[x] reaches scan[i] + 2 (n when there is none): doubling steps, then halving.
__global__ void k_sketch_compact_abund(const Rec* __restrict__ rec, const u64* __restrict__ scan, const u64 n, u64* __restrict__ out_keys, u32* __restrict__ out_abund) {
    const HeadFlag head{rec, n};
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        if (!head(i)) continue;
        const u64 at = scan[i], target = at + 2;
        u64 lo = i + 1, step = 1;   // scan[lo] = at + 1 < target
        while (lo + step <= n && scan[lo + step] < target) { lo += step; step <<= 1; }   // (at most 64 trips: step doubles)
        u64 hi = std::min(lo + step, n + 1);   // scan[hi] >= target, or hi = n + 1
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            if (scan[mid] < target) lo = mid; else hi = mid;
        }
        out_keys[at] = rec[i].hash;
        out_abund[at] = (u32)std::min<u64>(hi - 1 - i, 0xFFFFFFFFull);
    }
}

// off[s] = the heads of the sources before s, s = 0 .. n_sources
__global__ void k_sketch_offsets(const Rec* __restrict__ rec, const u64* __restrict__ scan, const u64 n, const u32 n_sources, u64* __restrict__ off) {
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s <= n_sources; s += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = n;   // the first entry whose source is >= s
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if (rec[mid].src < s) lo = mid + 1; else hi = mid;
        }
        off[s] = scan[lo];
    }
}

// the scratch the sort and the scan of n survivors ask for
int select_scratch(const u64 n, size_t* tb) {
    int rc = KSP_OK;
    size_t tb_sort = 0, tb_scan = 0;
    if (n) {
        KSP_TRY_HIP(rocprim::merge_sort(nullptr, tb_sort, (const Rec*)nullptr, (Rec*)nullptr, (size_t)n, RecBefore(), (hipStream_t) nullptr));
        KSP_TRY_HIP(rocprim::exclusive_scan(nullptr, tb_scan, head_flags_of(nullptr, 0), (u64*)nullptr, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
    }
    *tb = std::max<size_t>(std::max(tb_sort, tb_scan), 8);
done:
    return rc;
}

// The sketches on the CURRENT device; the arguments have passed ksp::check_sketch_args.  d_out_abund: the counts beside the keys, or NULL.
// mol 0: DNA; else the molecule type, the bytes being residues or, with `translate`, DNA read in six frames.
int sketch_on_device(const char* who, const uint8_t* d_seq, const u64 n_bytes, const u64* h_src_off, const u32 n_sources, const int ksize, const u64 max_hash,
                     const u32 seed, u64* d_out_keys, u32* d_out_abund, const u64 capacity, u64* h_out_off, ksp_sketch_stats* stats, const int mol = KSP_MOL_DNA,
                     const bool translate = false) {
    int rc = KSP_OK;
    ksp_sketch_stats S;
    std::memset(&S, 0, sizeof S);
    ksp::WorkgroupCap G;
    if ((rc = ksp::workgroup_cap("KSPIDER_SKETCH_MAX_WGS", who, G))) return rc;
    const u64 n_tiles = (n_bytes + kTile - 1) / kTile;
    ksp::DeviceArena A;
    u64 *d_src_off = nullptr, *d_out_off = nullptr, *d_scan = nullptr;
    Rec *d_recs = nullptr, *d_sorted = nullptr;
    unsigned long long* d_count = nullptr;
    void* d_tmp = nullptr;
    size_t tb = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    unsigned long long h_count[3] = {0, 0, 0};
    u64 n = 0, distinct = 0;
    // ---- everything the call holds, sized for `capacity` survivors and checked first
    if ((rc = select_scratch(capacity, &tb))) return rc;
    if ((rc = ksp::device_fits(who, 40ull * (capacity + 1) + tb + 16ull * ((u64)n_sources + 1) + 64,
                               "per survivor of the capacity 16 unsorted, 16 sorted and 8 of the scan, the sort's scratch, 16 per source")))
        return rc;
    if ((rc = A.alloc(&d_src_off, (size_t)n_sources + 1)) || (rc = A.alloc(&d_out_off, (size_t)n_sources + 1)) || (rc = A.alloc(&d_count, 3))) return rc;
    if (capacity && ((rc = A.alloc(&d_recs, (size_t)capacity)) || (rc = A.alloc(&d_sorted, (size_t)capacity)) || (rc = A.alloc(&d_scan, (size_t)capacity + 1)) ||
                     (rc = A.alloc_bytes(&d_tmp, tb))))
        return rc;
    KSP_TRY_HIP(hipMemcpy(d_src_off, h_src_off, ((size_t)n_sources + 1) * 8, hipMemcpyHostToDevice));
    KSP_TRY_HIP(hipMemset(d_count, 0, sizeof h_count));
    for (hipEvent_t& e : ev) KSP_TRY_HIP(hipEventCreate(&e));
    // ---- the hash pass
    KSP_TRY_HIP(hipEventRecord(ev[0], nullptr));
    if (n_tiles) {
        const HashArgs H{d_seq, n_bytes, n_tiles, d_src_off, n_sources, (u32)ksize, seed, max_hash, d_recs, d_recs ? capacity : 0, d_count};
        S.workgroups = G.grid_of(n_tiles);
        if (mol != KSP_MOL_DNA && translate) hipLaunchKernelGGL(k_sketch_hash_translated, dim3((unsigned)S.workgroups), dim3(kThreads), 0, nullptr, MolArgs{H, mol});
        else if (mol != KSP_MOL_DNA) hipLaunchKernelGGL(k_sketch_hash_protein, dim3((unsigned)S.workgroups), dim3(kThreads), 0, nullptr, MolArgs{H, mol});
        else if (ksize > 32) hipLaunchKernelGGL(k_sketch_hash<true>, dim3((unsigned)S.workgroups), dim3(kThreads), 0, nullptr, H);
        else hipLaunchKernelGGL(k_sketch_hash<false>, dim3((unsigned)S.workgroups), dim3(kThreads), 0, nullptr, H);
        KSP_TRY_HIP(hipGetLastError());
    }
    KSP_TRY_HIP(hipEventRecord(ev[1], nullptr));
    KSP_TRY_HIP(hipMemcpy(h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost));
    n = h_count[0];
    S.kept = S.needed = n; S.bases = h_count[1]; S.valid_kmers = h_count[2];
    KSP_TRY_HIP(hipEventElapsedTime(&S.ms_hash, ev[0], ev[1]));
    if (n > capacity) {
        if (stats) *stats = S;
        ksp::set_error(std::string(who) + ": " + std::to_string(n) + " survivors, room for " + std::to_string(capacity));
        rc = KSP_E_OVERFLOW;
        goto done;
    }
    // ---- the select pass
    if (n) {
        const unsigned ge = G.grid_of((n + 255) / 256);
        size_t b = tb;   // (sized for the capacity: fewer survivors must not ask for more)
        size_t need = 0;
        if ((rc = select_scratch(n, &need))) goto done;
        if (need > tb) { ksp::set_error(std::string(who) + ": fewer survivors ask for more scratch than the capacity"); rc = KSP_E_HIP; goto done; }
        KSP_TRY_HIP(rocprim::merge_sort(d_tmp, b, (const Rec*)d_recs, d_sorted, (size_t)n, RecBefore(), (hipStream_t) nullptr));
        b = tb;
        KSP_TRY_HIP(rocprim::exclusive_scan(d_tmp, b, head_flags_of(d_sorted, n), d_scan, (u64)0, (size_t)n + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        if (d_out_abund) hipLaunchKernelGGL(k_sketch_compact_abund, dim3(ge), dim3(256), 0, nullptr, (const Rec*)d_sorted, (const u64*)d_scan, n, d_out_keys, d_out_abund);
        else hipLaunchKernelGGL(k_sketch_compact, dim3(ge), dim3(256), 0, nullptr, (const Rec*)d_sorted, (const u64*)d_scan, n, d_out_keys);
        hipLaunchKernelGGL(k_sketch_offsets, dim3(G.grid_of(((u64)n_sources + 256) / 256)), dim3(256), 0, nullptr, (const Rec*)d_sorted, (const u64*)d_scan, n, n_sources,
                           d_out_off);
        KSP_TRY_HIP(hipGetLastError());
        KSP_TRY_HIP(hipEventRecord(ev[2], nullptr));
        KSP_TRY_HIP(hipMemcpy(h_out_off, d_out_off, ((size_t)n_sources + 1) * 8, hipMemcpyDeviceToHost));
        KSP_TRY_HIP(hipEventElapsedTime(&S.ms_select, ev[1], ev[2]));
        distinct = h_out_off[n_sources];
        if (h_out_off[0] != 0 || distinct == 0 || distinct > n) { ksp::set_error(std::string(who) + ": the select pass lost its keys"); rc = KSP_E_HIP; goto done; }
    } else {
        std::fill(h_out_off, h_out_off + (size_t)n_sources + 1, 0);
    }
    S.distinct_out = distinct;
    if (stats) *stats = S;
done:
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    return rc;
}

// the first capacity of ksp_sketch_host: $KSPIDER_SKETCH_FIRST_CAPACITY when it is set (tests: forces the retry), else `guess`
int env_first_capacity(const char* who, const u64 guess, u64* out) {
    const char* s = std::getenv("KSPIDER_SKETCH_FIRST_CAPACITY");
    *out = guess;
    if (!s || !*s) return KSP_OK;
    char* end = nullptr;
    const unsigned long long v = std::strtoull(s, &end, 10);
    if (end == s || *end || *s == '-') { ksp::set_error(std::string(who) + ": KSPIDER_SKETCH_FIRST_CAPACITY is a number"); return KSP_E_ARG; }
    *out = v;
    return KSP_OK;
}

int check_device_args(const char* who, const void* seq, const u64 n_bytes, const u64* src_off, const u32 n_sources, const int ksize, const void* out_off) {
    if (!out_off) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return ksp::check_sketch_args(who, seq, n_bytes, src_off, n_sources, ksize);
}

}  // namespace

void* ksp::pinned_alloc(const size_t bytes) {
    void* p = nullptr;
    return hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void ksp::pinned_free(void* p) {
    if (p) (void)hipHostFree(p);
}

// ksp_sketch_device, with counts ksp_sketch_device_abund, and with a molecule type and flags ksp_sketch_device_mol
static int sketch_device(const char* who, const bool counted, int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize,
                  uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint32_t* d_out_abund, uint64_t capacity, uint64_t* h_out_offsets, ksp_sketch_stats* stats,
                  const int mol = KSP_MOL_DNA, const uint64_t flags = 0) {
    if (const int rc = ksp::check_sketch_mol(who, ksize, mol, flags)) return rc;
    if (const int rc = check_device_args(who, d_seq, n_bytes, h_src_offsets, n_sources, ksize, h_out_offsets)) return rc;
    if (!d_out_keys && capacity) { ksp::set_error(std::string(who) + ": d_out_keys is NULL but capacity is not 0"); return KSP_E_ARG; }
    if (counted && !d_out_abund && capacity) { ksp::set_error(std::string(who) + ": d_out_abund is NULL but capacity is not 0"); return KSP_E_ARG; }
    if ((uintptr_t)d_seq & 15) { ksp::set_error(std::string(who) + ": d_seq is not 16-byte aligned"); return KSP_E_ARG; }
    if (const int rc = ksp::set_device(who, device)) return rc;
    return sketch_on_device(who, d_seq, n_bytes, h_src_offsets, n_sources, ksize, max_hash, seed, d_out_keys, counted ? d_out_abund : nullptr, capacity, h_out_offsets, stats, mol,
                            (flags & KSP_SKETCH_TRANSLATE) != 0);
}

// ksp_sketch_host, with counts in *out_abund ksp_sketch_host_abund, and with a molecule type and flags ksp_sketch_host_mol
static int sketch_host(const char* who, int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, uint64_t max_hash, uint32_t seed,
                uint64_t** out_keys, uint32_t** out_abund, uint64_t* out_offsets, ksp_sketch_stats* stats, const int mol = KSP_MOL_DNA, const uint64_t flags = 0) {
    if (const int rc = ksp::check_sketch_mol(who, ksize, mol, flags)) return rc;
    if (const int rc = check_device_args(who, seq, n_bytes, src_offsets, n_sources, ksize, out_offsets)) return rc;
    const bool translate = (flags & KSP_SKETCH_TRANSLATE) != 0;
    u64 first = 0;
    {   // the share of all hashes that max_hash keeps, a quarter more, and room for a small input whatever its luck; a translated
        // position has two hashes
        const double share = ((double)max_hash + 1.0) / 18446744073709551616.0;
        const u64 per = translate ? 2 : 1;
        const u64 guess = std::min<u64>(per * n_bytes, per * ((u64)((double)n_bytes * share * 1.25) + 4096));
        if (const int rc = env_first_capacity(who, guess, &first)) return rc;
    }
    if (const int rc = ksp::set_device(who, device)) return rc;
    int rc = KSP_OK;
    ksp::DeviceArena A;
    uint8_t* d_seq = nullptr;
    u64 *d_keys = nullptr, *h_keys = nullptr, capacity = first;
    u32 *d_abund = nullptr, *h_abund = nullptr;
    const u64 per_key = out_abund ? 12 : 8;
    ksp_sketch_stats S;
    float ms_upload = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::memset(&S, 0, sizeof S);
    if ((rc = ksp::device_fits(who, n_bytes + 16 + per_key * capacity, out_abund ? "the bytes and the first key and count buffers" : "the bytes and the first key buffer"))) return rc;
    if ((rc = A.alloc(&d_seq, (size_t)n_bytes + 16)) || (rc = A.alloc(&d_keys, (size_t)capacity))) return rc;
    if (out_abund && (rc = A.alloc(&d_abund, (size_t)capacity + 1))) return rc;
    KSP_TRY_HIP(hipEventCreate(&ev0));
    KSP_TRY_HIP(hipEventCreate(&ev1));
    KSP_TRY_HIP(hipEventRecord(ev0, nullptr));
    if (n_bytes) KSP_TRY_HIP(hipMemcpyAsync(d_seq, seq, (size_t)n_bytes, hipMemcpyHostToDevice, nullptr));
    KSP_TRY_HIP(hipEventRecord(ev1, nullptr));
    KSP_TRY_HIP(hipEventSynchronize(ev1));
    KSP_TRY_HIP(hipEventElapsedTime(&ms_upload, ev0, ev1));
    rc = sketch_on_device(who, d_seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, d_keys, d_abund, capacity, out_offsets, &S, mol, translate);
    if (rc == KSP_E_OVERFLOW) {   // once more, at the exact size
        KSP_TRY_HIP(A.release(d_keys));
        d_keys = nullptr;
        if (d_abund) KSP_TRY_HIP(A.release(d_abund));
        d_abund = nullptr;
        capacity = S.needed;
        if ((rc = ksp::device_fits(who, per_key * capacity, out_abund ? "the keys and the counts" : "the keys"))) goto done;
        if ((rc = A.alloc(&d_keys, (size_t)capacity))) goto done;
        if (out_abund && (rc = A.alloc(&d_abund, (size_t)capacity + 1))) goto done;
        rc = sketch_on_device(who, d_seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, d_keys, d_abund, capacity, out_offsets, &S, mol, translate);
        S.retries = 1;
    }
    if (rc != KSP_OK) goto done;
    h_keys = (u64*)std::malloc((size_t)std::max<u64>(S.distinct_out, 1) * 8);
    if (out_abund) h_abund = (u32*)std::malloc((size_t)std::max<u64>(S.distinct_out, 1) * 4);
    if (!h_keys || (out_abund && !h_abund)) { ksp::set_error(std::string(who) + ": out of host memory"); rc = KSP_E_LIMIT; goto done; }
    if (S.distinct_out) KSP_TRY_HIP(hipMemcpy(h_keys, d_keys, (size_t)S.distinct_out * 8, hipMemcpyDeviceToHost));
    if (S.distinct_out && out_abund) KSP_TRY_HIP(hipMemcpy(h_abund, d_abund, (size_t)S.distinct_out * 4, hipMemcpyDeviceToHost));
    *out_keys = h_keys;
    h_keys = nullptr;
    if (out_abund) { *out_abund = h_abund; h_abund = nullptr; }
    S.ms_upload = ms_upload;
    if (stats) *stats = S;
done:
    if (h_keys) std::free(h_keys);
    if (h_abund) std::free(h_abund);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    return rc;
}

extern "C" int ksp_sketch_device(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize,
                                 uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint64_t capacity, uint64_t* h_out_offsets,
                                 ksp_sketch_stats* stats) {
    return sketch_device("ksp_sketch_device", false, device, d_seq, n_bytes, h_src_offsets, n_sources, ksize, max_hash, seed, d_out_keys, nullptr, capacity, h_out_offsets, stats);
}

extern "C" int ksp_sketch_device_abund(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize,
                                       uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint32_t* d_out_abund, uint64_t capacity, uint64_t* h_out_offsets,
                                       ksp_sketch_stats* stats) {
    return sketch_device("ksp_sketch_device_abund", true, device, d_seq, n_bytes, h_src_offsets, n_sources, ksize, max_hash, seed, d_out_keys, d_out_abund, capacity, h_out_offsets,
                         stats);
}

extern "C" int ksp_sketch_host(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize,
                               uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint64_t* out_offsets, ksp_sketch_stats* stats) {
    const char* who = "ksp_sketch_host";
    if (!out_keys) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return sketch_host(who, device, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, nullptr, out_offsets, stats);
}

extern "C" int ksp_sketch_host_abund(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize,
                                     uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint32_t** out_abund, uint64_t* out_offsets, ksp_sketch_stats* stats) {
    const char* who = "ksp_sketch_host_abund";
    if (!out_keys || !out_abund) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return sketch_host(who, device, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, out_abund, out_offsets, stats);
}

extern "C" int ksp_sketch_device_mol(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize, int moltype, uint64_t flags,
                                     uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint32_t* d_out_abund, uint64_t capacity, uint64_t* h_out_offsets,
                                     ksp_sketch_stats* stats) {
    return sketch_device("ksp_sketch_device_mol", d_out_abund != nullptr, device, d_seq, n_bytes, h_src_offsets, n_sources, ksize, max_hash, seed, d_out_keys, d_out_abund, capacity,
                         h_out_offsets, stats, moltype, flags);
}

extern "C" int ksp_sketch_host_mol(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, int moltype, uint64_t flags,
                                   uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint32_t** out_abund, uint64_t* out_offsets, ksp_sketch_stats* stats) {
    const char* who = "ksp_sketch_host_mol";
    if (!out_keys) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return sketch_host(who, device, seq, n_bytes, src_offsets, n_sources, ksize, max_hash, seed, out_keys, out_abund, out_offsets, stats, moltype, flags);
}
