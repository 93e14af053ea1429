// The table side of query mode, shared by query.hip and gather.hip: one tile's collision-free sorted table of the
// query hashes with its directory, the look-up a probing lane does in it, the host sequence that builds it, and the front of a
// call that both share: the probe sources split by run length, the offsets and the lists uploaded, the host keys uploaded.
//
//   table    per tile of at most KSP_QUERY_TILE consecutive queries: every query entry tagged with its query index inside the
//            tile (k_query_tag), (key, tag) sorted by key with rocPRIM's radix sort (stable: the tags of a key ascend), adjacent
//            duplicates dropped by one scan of packed (head, kept) flags and k_query_compact.  Result: the distinct keys tk[U],
//            the holder ranges toff[U + 1] and the holders tq[].  First level: dir[b] = the first index whose key >> shift is
//            >= b (k_query_dir; bits and shift: ksp_query_directory), then a binary search inside the bucket.  A probe key above
//            tk[U - 1] misses without a memory access.  No hash function, no compare-and-swap build, no collisions.
// Everything here has internal linkage: each of the two translation units gets its own copy.
#ifndef KSPIDER_QUERY_TABLE_HIP_H
#define KSPIDER_QUERY_TABLE_HIP_H
#include <cstdint>
#include <cstdlib>
#include <algorithm>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"

namespace {

typedef uint32_t u32;
typedef uint64_t u64;

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

// the tiles of `tile` consecutive queries and the entries of the largest of them; KSP_E_LIMIT for a tile of 2^31 entries or more
int query_tiles(const char* who, const u64* h_q_off, const u32 n_q, const u64 tile, u32* n_tiles, u64* e_max) {
    *n_tiles = (u32)(((u64)n_q + tile - 1) / tile);
    *e_max = 0;
    for (u32 t = 0; t < *n_tiles; ++t) {
        const u64 q0 = (u64)t * tile, q1 = std::min<u64>(q0 + tile, n_q), E = h_q_off[q1] - h_q_off[q0];
        if (E >= (1ull << 31)) { ksp::set_error(std::string(who) + ": a query tile of 2^31 entries or more (lower KSP_QUERY_TILE)"); return KSP_E_LIMIT; }
        *e_max = std::max(*e_max, E);
    }
    return KSP_OK;
}

// The sources 0 .. n - 1 that have entries (one without shares nothing), numbered from `first`, appended to probes[0] when the run
// is shorter than long_run entries and to probes[1] otherwise.
void query_split_sources(const u64* h_off, const u32 n, const u64 long_run, const u32 first, std::vector<u32> (&probes)[2]) {
    for (u32 p = 0; p < n; ++p)
        if (const u64 len = h_off[p + 1] - h_off[p]) probes[len >= long_run].push_back(first + p);
}

// both offset arrays as *d_db_off, *d_q_off and every non-empty list as d_list[c] in the arena (an empty list stays NULL)
int query_upload_front(ksp::DeviceArena& A, const u64* h_db_off, const u32 n_db, const u64* h_q_off, const u32 n_q, const std::vector<u32> (&probes)[2], u64** d_db_off,
                       u64** d_q_off, u32* (&d_list)[2]) {
    int rc = KSP_OK;
    if ((rc = A.alloc(d_db_off, (size_t)n_db + 1)) || (rc = A.alloc(d_q_off, (size_t)n_q + 1))) return rc;
    for (int c = 0; c < 2; ++c)
        if (!probes[c].empty() && (rc = A.alloc(&d_list[c], probes[c].size()))) return rc;
    KSP_HIP(hipMemcpy(*d_db_off, h_db_off, ((size_t)n_db + 1) * 8, hipMemcpyHostToDevice));
    KSP_HIP(hipMemcpy(*d_q_off, h_q_off, ((size_t)n_q + 1) * 8, hipMemcpyHostToDevice));
    for (int c = 0; c < 2; ++c)
        if (!probes[c].empty()) KSP_HIP(hipMemcpy(d_list[c], probes[c].data(), probes[c].size() * 4, hipMemcpyHostToDevice));
    return KSP_OK;
}

// the host keys of both sides as *d_db, *d_q in the arena (an entry more than the keys: never an allocation of 0 bytes)
int query_upload_keys(ksp::DeviceArena& A, const u64* db_keys, const u64 n_dbk, const u64* q_keys, const u64 n_qk, u64** d_db, u64** d_q) {
    int rc = KSP_OK;
    if ((rc = A.alloc(d_db, (size_t)n_dbk + 1)) || (rc = A.alloc(d_q, (size_t)n_qk + 1))) return rc;
    KSP_HIP(hipMemcpy(*d_db, db_keys, (size_t)n_dbk * 8, hipMemcpyHostToDevice));
    KSP_HIP(hipMemcpy(*d_q, q_keys, (size_t)n_qk * 8, hipMemcpyHostToDevice));
    return KSP_OK;
}

// What the table of the largest tile (e_max entries) holds on the device: per entry 40 bytes (tag 4, sorted key 8 and tag 4,
// scan 8, table key 8, holder range 4, holder 4), the directory, and the library's scratch, which the caller owns (it may be
// larger than the table's need and serve the caller's own sorts).
struct QTableBufs {
    u64 e_max = 0;
    u64 *skey = nullptr, *scan = nullptr, *tk = nullptr;
    u32 *tag = nullptr, *stag = nullptr, *toff = nullptr, *tq = nullptr, *dir = nullptr;
    void* tmp = nullptr;
    size_t tb = 0;
    static u64 dir_max() { return (1ull << KSP_QUERY_DIR_BITS_MAX) + 1; }
    u64 dir_entries() const { return std::min<u64>(dir_max(), e_max + 2); }
    u64 bytes() const { return 40ull * (e_max + 1) + 4 * dir_entries(); }   // (without the scratch)
};

inline auto query_flags_of(const u64* k, const u32* t, const u32 E) {
    return rocprim::make_transform_iterator(rocprim::counting_iterator<u32>(0), QFlags{k, t, E});
}

// *tb = the scratch the sort and the scan of a table of E entries ask for
int query_table_scratch(const u64 E, size_t* tb) {
    size_t tb_sort = 0, tb_scan = 0;
    if (E) {
        KSP_HIP(rocprim::radix_sort_pairs(nullptr, tb_sort, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)E, 0, 64, (hipStream_t) nullptr));
        KSP_HIP(rocprim::exclusive_scan(nullptr, tb_scan, query_flags_of(nullptr, nullptr, 0), (u64*)nullptr, (u64)0, (size_t)E + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
    }
    *tb = std::max(tb_sort, tb_scan);
    return KSP_OK;
}

// the table's arrays in the arena (B.e_max > 0 is set; the scratch is the caller's)
int query_table_alloc(ksp::DeviceArena& A, QTableBufs& B) {
    int rc = KSP_OK;
    if ((rc = A.alloc(&B.tag, (size_t)B.e_max)) || (rc = A.alloc(&B.skey, (size_t)B.e_max)) || (rc = A.alloc(&B.stag, (size_t)B.e_max)) || (rc = A.alloc(&B.scan, (size_t)B.e_max + 1)) ||
        (rc = A.alloc(&B.tk, (size_t)B.e_max)) || (rc = A.alloc(&B.toff, (size_t)B.e_max + 1)) || (rc = A.alloc(&B.tq, (size_t)B.e_max)) ||
        (rc = A.alloc(&B.dir, (size_t)B.dir_entries())))
        return rc;
    return KSP_OK;
}

// The table of the tile q0 .. q0 + nq - 1, which has E > 0 entries from e0 on: *T, its U distinct keys and H holders.  Waits for
// the device twice (the totals of the scan, the largest key).
int query_table_build(const char* who, const ksp::WorkgroupCap& G, const QTableBufs& B, const u64* d_q_keys, const u64* d_q_off, const u32 q0, const u32 nq, const u64 e0,
                      const u32 E, QTable* T, u32* U_out, u32* H_out) {
    const unsigned ge = G.grid_of(((u64)E + 255) / 256);
    u64 totals = 0, max_key = 0;
    u32 U = 0, H = 0, n_buckets = 0;
    int bits = 0, shift = 0;
    hipLaunchKernelGGL(k_query_tag, dim3(ge), dim3(256), 0, nullptr, d_q_off, q0, nq, e0, E, B.tag);
    KSP_HIP(hipGetLastError());
    {
        size_t b = 0;   // (the scratch was sized for the largest tile: a smaller one must not ask for more)
        if (const int rc = query_table_scratch(E, &b)) return rc;
        if (b > B.tb) { ksp::set_error(std::string(who) + ": a smaller tile asks for more scratch than the largest"); return KSP_E_HIP; }
        b = B.tb;
        KSP_HIP(rocprim::radix_sort_pairs(B.tmp, b, d_q_keys + e0, B.skey, (const u32*)B.tag, B.stag, (size_t)E, 0, 64, (hipStream_t) nullptr));
        b = B.tb;
        KSP_HIP(rocprim::exclusive_scan(B.tmp, b, query_flags_of(B.skey, B.stag, E), B.scan, (u64)0, (size_t)E + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
    }
    KSP_HIP(hipMemcpy(&totals, B.scan + E, 8, hipMemcpyDeviceToHost));
    U = (u32)(totals >> 32);
    H = (u32)totals;
    if (U == 0 || U > E || H < U || H > E) { ksp::set_error(std::string(who) + ": the query table lost its keys"); return KSP_E_HIP; }
    hipLaunchKernelGGL(k_query_compact, dim3(ge), dim3(256), 0, nullptr, (const u64*)B.skey, (const u32*)B.stag, (const u64*)B.scan, E, B.tk, B.toff, B.tq);
    KSP_HIP(hipGetLastError());
    KSP_HIP(hipMemcpy(&max_key, B.tk + (U - 1), 8, hipMemcpyDeviceToHost));
    (void)ksp_query_directory(max_key, U, &bits, &shift);
    n_buckets = 1u << bits;
    if ((u64)n_buckets + 1 > B.dir_entries()) { ksp::set_error(std::string(who) + ": the directory outgrew its buffer"); return KSP_E_HIP; }
    hipLaunchKernelGGL(k_query_dir, dim3(G.grid_of(((u64)n_buckets + 256) / 256)), dim3(256), 0, nullptr, (const u64*)B.tk, U, shift, n_buckets, B.dir);
    KSP_HIP(hipGetLastError());
    *T = QTable{B.tk, B.toff, B.tq, B.dir, max_key, shift, q0, nq};
    *U_out = U;
    *H_out = H;
    return KSP_OK;
}

}  // namespace
#endif
