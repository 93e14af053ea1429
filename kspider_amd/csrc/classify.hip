// The device part of classify: records of DNA in batches against one table of all references.
//
//   table    once per session: the reference hashes <= max_hash with their reference index as the tag, query mode's table
//            (query_table.hip.h: query_table_build) over all of them as ONE tile — no per-query LDS counters exist on this path,
//            so the number of references is not bounded by KSP_QUERY_TILE_MAX.  What the build needed beside the table is freed.
//   hash     per batch, classify_kernels.hip.h: k_classify_hash leaves one word (record << 32) | table_index per kept window
//            that hits, behind the words the session already holds, and counts the words past the room without writing there.
//            A batch that does not fit: the held words are sorted and made unique, then the buffer grows to the counted need,
//            and the kernel runs again with its tallies off.
//   finish   rocPRIM radix sort and unique of the words; matched[record] = its words; every word expanded into
//            (record << 32) | reference for each holder tq[toff[u] .. toff[u + 1]) of its key; radix sort; run lengths = hits;
//            the cut at min_hits by one scan; the per-record summary by one thread per record over its runs.
// Every loop is bounded by a size the host computed; no workgroup waits on another; every value is an integer sum or a sorted
// list, so nothing depends on scheduling.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"
#include "query_table.hip.h"
#include "sketch_hash.h"

namespace {

namespace sk = ksp_sketch;

#define KSP_SKETCH_PARTS_ONLY   // the staging, the break mask, kmer_at, window_in_source: not the sketcher's frame and kernels
#include "sketch_kernels.hip.h"
#include "classify_kernels.hip.h"

// matched[record] += 1 for every distinct word
__global__ void k_classify_matched(const u64* __restrict__ words, const u64 n, u32* __restrict__ matched) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) atomicAdd(&matched[words[i] >> 32], 1u);
}

// the holders of word i's key, 0 behind the end
struct HolderCount {
    const u64* words;
    const u32* toff;
    u64 n;
    __host__ __device__ u64 operator()(const u64 i) const {
        if (i >= n) return 0;
        const u32 u = (u32)words[i];
        return (u64)(toff[u + 1] - toff[u]);
    }
};
inline auto holder_counts_of(const u64* words, const u32* toff, const u64 n) {
    return rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), HolderCount{words, toff, n});
}

// scan[i] = the pairs of the words before i (n + 1 values).  pairs[j] = (record << 32) | reference: j belongs to the last word
// whose scan is <= j, and is its (j - scan)-th holder.
__global__ void k_classify_expand(const u64* __restrict__ words, const u64* __restrict__ scan, const u64 n, const u32* __restrict__ toff, const u32* __restrict__ tq,
                                  const u64 n_pairs, u64* __restrict__ pairs) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_pairs; j += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = n;   // scan[lo] <= j < scan[hi]
        while (hi - lo > 1) {
            const u64 mid = lo + (hi - lo) / 2;
            if (scan[mid] <= j) lo = mid; else hi = mid;
        }
        const u64 w = words[lo];
        pairs[j] = (w & 0xFFFFFFFF00000000ull) | (u64)tq[toff[(u32)w] + (u32)(j - scan[lo])];
    }
}

// 1 for a run of at least min_hits, 0 behind the end
struct RowFlag {
    const u32* hits;
    u64 n;
    u32 min_hits;
    __host__ __device__ u64 operator()(const u64 i) const { return i < n && hits[i] >= min_hits; }
};
inline auto row_flags_of(const u32* hits, const u64 n, const u32 min_hits) {
    return rocprim::make_transform_iterator(rocprim::counting_iterator<u64>(0), RowFlag{hits, n, min_hits});
}

// scan[i] = rows before run i
__global__ void k_classify_rows(const u64* __restrict__ run, const u32* __restrict__ hits, const u64* __restrict__ scan, const u64 n, const u32 min_hits,
                                ksp_classify_row* __restrict__ rows) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (hits[i] >= min_hits) rows[scan[i]] = ksp_classify_row{(u32)(run[i] >> 32), (u32)run[i], hits[i], 0};
}

// one thread per record over its runs (they are sorted by (record, reference): the first of the largest is the smaller reference)
__global__ void k_classify_summary(const u64* __restrict__ run, const u32* __restrict__ hits, const u64 n, const u32 min_hits, const u32 n_records,
                                   u32* __restrict__ n_refs_hit, u32* __restrict__ best_ref, u32* __restrict__ best_hits, u32* __restrict__ second_hits) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_records; r += (u64)gridDim.x * blockDim.x) {
        u64 lo = 0, hi = n;   // the first run of a record >= r
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if ((run[mid] >> 32) < r) lo = mid + 1; else hi = mid;
        }
        u32 refs = 0, ref = 0xFFFFFFFFu, best = 0, second = 0;
        for (u64 i = lo; i < n && (run[i] >> 32) == r; ++i) {
            const u32 h = hits[i];
            if (h < min_hits) continue;
            ++refs;
            if (h > best) { second = best; best = h; ref = (u32)run[i]; }
            else if (h > second) second = h;
        }
        n_refs_hit[r] = refs; best_ref[r] = ref; best_hits[r] = best; second_hits[r] = second;
    }
}

// the scratch rocPRIM asks for a sort and a unique of n words
int words_scratch(const u64 n, size_t* tb) {
    size_t a = 0, b = 0;
    if (n) {
        KSP_HIP(rocprim::radix_sort_keys(nullptr, a, (const u64*)nullptr, (u64*)nullptr, (size_t)n, 0, 64, (hipStream_t) nullptr));
        KSP_HIP(rocprim::unique(nullptr, b, (const u64*)nullptr, (u64*)nullptr, (u64*)nullptr, (size_t)n, rocprim::equal_to<u64>(), (hipStream_t) nullptr));
    }
    *tb = std::max<size_t>(std::max(a, b), 8);
    return KSP_OK;
}

// d_words[0 .. n) sorted and made unique in place: *n_out words.  Asks for 8 n bytes and the library's scratch first.
int sort_unique_words(const char* who, u64* d_words, const u64 n, u64* n_out) {
    *n_out = n;
    if (n == 0) return KSP_OK;
    int rc = KSP_OK;
    size_t tb = 0, b = 0;
    if ((rc = words_scratch(n, &tb))) return rc;
    if ((rc = ksp::device_fits(who, 8 * n + tb + 8, "the sort of the hit words: 8 per word and the sort's scratch"))) return rc;
    ksp::DeviceArena A;
    u64 *d_sorted = nullptr, *d_n = nullptr;
    void* d_tmp = nullptr;
    if ((rc = A.alloc(&d_sorted, (size_t)n)) || (rc = A.alloc(&d_n, 1)) || (rc = A.alloc_bytes(&d_tmp, tb))) return rc;
    b = tb;
    KSP_HIP(rocprim::radix_sort_keys(d_tmp, b, (const u64*)d_words, d_sorted, (size_t)n, 0, 64, (hipStream_t) nullptr));
    b = tb;
    KSP_HIP(rocprim::unique(d_tmp, b, (const u64*)d_sorted, d_words, d_n, (size_t)n, rocprim::equal_to<u64>(), (hipStream_t) nullptr));
    KSP_HIP(hipMemcpy(n_out, d_n, 8, hipMemcpyDeviceToHost));
    if (*n_out == 0 || *n_out > n) { ksp::set_error(std::string(who) + ": the sort of the hit words lost them"); return KSP_E_HIP; }
    return KSP_OK;
}

}  // namespace

struct ksp_classify {
    int device = 0, ksize = 0;
    u64 max_hash = 0;
    u32 seed = 0, n_refs = 0;
    ksp::DeviceArena table_mem;   // tk, toff, tq, dir
    QTable T{};                   // T.nq = 0: no reference hash can be hit, there is no table
    u64* d_hits = nullptr;        // hit_cap words, the first `held` of them in use
    u64 hit_cap = 0, held = 0;
    u32* d_kept = nullptr;        // kept windows of the records 0 .. kept_cap - 1
    u64 kept_cap = 0, n_seen = 0; // n_seen: the largest record id added + 1
    unsigned long long* d_count = nullptr;   // the hash pass's four counters
    ksp::Buf seq, seg_off, seg_rec;          // the batch on the device
    ksp_classify_stats st;
    bool finished = false, failed = false;
    ~ksp_classify() {
        if (d_hits) (void)hipFree(d_hits);
        if (d_kept) (void)hipFree(d_kept);
        if (d_count) (void)hipFree(d_count);
        seq.release(); seg_off.release(); seg_rec.release();
    }
};

namespace {

int classify_open(const char* who, const int device, const int ksize, const u64 max_hash, const u32 seed, const u64* ref_keys, const u64* ref_off, const u32 n_refs,
                  ksp_classify** out) {
    int rc = KSP_OK;
    if (!out) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    *out = nullptr;
    if ((rc = ksp::check_classify_refs(who, ksize, ref_keys, ref_off, n_refs))) return rc;
    u64 first = 0;
    if ((rc = env_number(who, "KSPIDER_CLASSIFY_FIRST_CAPACITY", 1ull << 20, 1, 1ull << 40, &first))) return rc;
    // the reference hashes that can be hit
    std::vector<u64> keys, off((size_t)n_refs + 1, 0);
    try {
        for (u32 q = 0; q < n_refs; ++q) {
            const u64* b = ref_keys + ref_off[q];
            keys.insert(keys.end(), b, std::upper_bound(b, ref_keys + ref_off[q + 1], max_hash));
            off[q + 1] = keys.size();
        }
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
    const u64 E = keys.size();
    if (E >= (1ull << 31)) { ksp::set_error(std::string(who) + ": the references hold 2^31 entries or more"); return KSP_E_LIMIT; }
    if ((rc = ksp::set_device(who, device))) return rc;
    ksp::WorkgroupCap G;
    if ((rc = ksp::workgroup_cap("KSPIDER_SKETCH_MAX_WGS", who, G))) return rc;
    ksp_classify* c = new (std::nothrow) ksp_classify;
    if (!c) { ksp::set_error(std::string(who) + ": out of host memory"); return KSP_E_LIMIT; }
    std::memset(&c->st, 0, sizeof c->st);
    c->device = device; c->ksize = ksize; c->max_hash = max_hash; c->seed = seed; c->n_refs = n_refs;
    const auto fail = [&](const int code) { delete c; return code; };
    QTableBufs B;
    B.e_max = E;
    if ((rc = query_table_scratch(E, &B.tb))) return fail(rc);
    B.tb = std::max<size_t>(B.tb, 8);
    // ---- everything the session holds at first, asked for before anything runs
    if ((rc = ksp::device_fits(who, (E ? B.bytes() + B.tb + 8 * (E + 1) + 8 * ((u64)n_refs + 1) : 0) + 8 * first + 64,
                               "per reference hash 40 of the table's build and 8 of the upload, the directory, the sort's scratch, 8 per reference, 8 per hit word of the first capacity")))
        return fail(rc);
    if (hipMalloc(&c->d_hits, (size_t)first * 8) != hipSuccess || hipMalloc(&c->d_count, 4 * sizeof(unsigned long long)) != hipSuccess) {
        ksp::set_error(std::string(who) + ": hipMalloc of the hit words");
        return fail(KSP_E_HIP);
    }
    c->hit_cap = first;
    if (E) {
        ksp::DeviceArena tmp;   // what only the build needs
        ksp::Events<2> ev;
        u64 *d_keys = nullptr, *d_off = nullptr;
        u32 U = 0, H = 0;
        if ((rc = ev.create())) return fail(rc);
        if ((rc = tmp.alloc(&B.tag, (size_t)E)) || (rc = tmp.alloc(&B.skey, (size_t)E)) || (rc = tmp.alloc(&B.stag, (size_t)E)) || (rc = tmp.alloc(&B.scan, (size_t)E + 1)) ||
            (rc = tmp.alloc_bytes(&B.tmp, B.tb)) || (rc = tmp.alloc(&d_keys, (size_t)E)) || (rc = tmp.alloc(&d_off, (size_t)n_refs + 1)) ||
            (rc = c->table_mem.alloc(&B.tk, (size_t)E)) || (rc = c->table_mem.alloc(&B.toff, (size_t)E + 1)) || (rc = c->table_mem.alloc(&B.tq, (size_t)E)) ||
            (rc = c->table_mem.alloc(&B.dir, (size_t)B.dir_entries())))
            return fail(rc);
        const auto hip = [&](const hipError_t e, const char* what) {
            if (e == hipSuccess) return false;
            ksp::set_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
            return true;
        };
        if (hip(hipMemcpy(d_keys, keys.data(), (size_t)E * 8, hipMemcpyHostToDevice), "upload of the reference hashes") ||
            hip(hipMemcpy(d_off, off.data(), ((size_t)n_refs + 1) * 8, hipMemcpyHostToDevice), "upload of the reference offsets") || hip(hipEventRecord(ev[0], nullptr), "hipEventRecord"))
            return fail(KSP_E_HIP);
        if ((rc = query_table_build(who, G, B, d_keys, d_off, 0, n_refs, 0, (u32)E, &c->T, &U, &H))) return fail(rc);
        if (hip(hipEventRecord(ev[1], nullptr), "hipEventRecord") || hip(hipEventSynchronize(ev[1]), "the table's build") ||
            hip(hipEventElapsedTime(&c->st.ms_table, ev[0], ev[1]), "hipEventElapsedTime"))
            return fail(KSP_E_HIP);
        c->st.table_keys = U;
        c->st.table_holders = H;
    }
    *out = c;
    return KSP_OK;
}

// one run of the hash pass over the batch that is on the device: *n_hits = the hit words it has (written only as far as there is room)
int classify_launch(ksp_classify* c, const ksp::WorkgroupCap& G, const u64 n_bytes, const u32 n_seg, const bool tally, u64* n_hits, unsigned long long (&h_count)[4]) {
    const u64 n_tiles = (n_bytes + kTile - 1) / kTile;
    KSP_HIP(hipMemset(c->d_count, 0, sizeof h_count));
    if (n_tiles) {
        ClassifyArgs C;
        C.h = HashArgs{c->seq.as<uint8_t>(), n_bytes, n_tiles, c->seg_off.as<u64>(), n_seg, (u32)c->ksize, c->seed, c->max_hash, nullptr, 0, c->d_count};
        C.T = c->T;
        C.seg_rec = c->seg_rec.as<u32>();
        C.kept_windows = c->d_kept;
        C.hits = (unsigned long long*)(c->d_hits + c->held);
        C.hit_capacity = c->hit_cap - c->held;
        C.tally = tally ? 1u : 0u;
        const unsigned grid = G.grid_of(n_tiles);
        c->st.workgroups = std::max<u64>(c->st.workgroups, grid);
        if (c->ksize > 32) hipLaunchKernelGGL(k_classify_hash<true>, dim3(grid), dim3(kThreads), 0, nullptr, C);
        else hipLaunchKernelGGL(k_classify_hash<false>, dim3(grid), dim3(kThreads), 0, nullptr, C);
        KSP_HIP(hipGetLastError());
    }
    KSP_HIP(hipMemcpy(h_count, c->d_count, sizeof h_count, hipMemcpyDeviceToHost));
    *n_hits = h_count[0];
    return KSP_OK;
}

int classify_add(const char* who, ksp_classify* c, const uint8_t* seq, const u64 n_bytes, const u64* seg_off, const u32* seg_rec, const u32 n_seg) {
    int rc = KSP_OK;
    if (!c) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if (c->finished || c->failed) { ksp::set_error(std::string(who) + (c->failed ? ": the session has failed" : ": the session is finished")); return KSP_E_ARG; }
    if ((rc = ksp::check_classify_batch(who, seq, n_bytes, seg_off, seg_rec, n_seg))) return rc;
    if ((rc = ksp::set_device(who, c->device))) return rc;
    ksp::WorkgroupCap G;
    if ((rc = ksp::workgroup_cap("KSPIDER_SKETCH_MAX_WGS", who, G))) return rc;
    std::vector<u32> iota;
    u64 n_seen = c->n_seen;
    try {
        if (!seg_rec) {
            iota.resize(n_seg);
            for (u32 s = 0; s < n_seg; ++s) iota[s] = s;
            seg_rec = iota.data();
        }
    } catch (const std::bad_alloc&) {
        ksp::set_error(std::string(who) + ": out of host memory");
        return KSP_E_LIMIT;
    }
    for (u32 s = 0; s < n_seg; ++s) n_seen = std::max<u64>(n_seen, (u64)seg_rec[s] + 1);
    // ---- what the batch needs beyond what the session holds, asked for before anything runs
    const u64 kept_want = n_seen > c->kept_cap ? std::max<u64>(n_seen, 2 * c->kept_cap) : c->kept_cap;
    {
        u64 more = 0;
        if (n_bytes + 16 > c->seq.bytes) more += (n_bytes + 16) * 9 / 8 + 256;
        if (8 * ((u64)n_seg + 1) > c->seg_off.bytes) more += 8 * ((u64)n_seg + 1) * 9 / 8 + 256;
        if (4 * (u64)n_seg > c->seg_rec.bytes) more += 4 * (u64)n_seg * 9 / 8 + 256;
        if (kept_want > c->kept_cap) more += 4 * kept_want;
        if (more && (rc = ksp::device_fits(who, more, "the batch's bytes and 12 per segment, 4 per record"))) return rc;
    }
    if (kept_want > c->kept_cap) {
        u32* grown = nullptr;
        KSP_HIP(hipMalloc(&grown, (size_t)kept_want * 4));
        if (hipMemset(grown, 0, (size_t)kept_want * 4) != hipSuccess || (c->kept_cap && hipMemcpy(grown, c->d_kept, (size_t)c->kept_cap * 4, hipMemcpyDeviceToDevice) != hipSuccess)) {
            (void)hipFree(grown);
            ksp::set_error(std::string(who) + ": the kept-window counters could not be grown");
            return KSP_E_HIP;
        }
        if (c->d_kept) (void)hipFree(c->d_kept);
        c->d_kept = grown;
        c->kept_cap = kept_want;
    }
    if ((rc = c->seq.ensure((size_t)n_bytes + 16)) || (rc = c->seg_off.ensure(8 * ((size_t)n_seg + 1))) || (rc = c->seg_rec.ensure(4 * (size_t)n_seg))) return rc;
    ksp::Events<2> ev;
    if ((rc = ev.create())) return rc;
    if (n_bytes) KSP_HIP(hipMemcpyAsync(c->seq.p, seq, (size_t)n_bytes, hipMemcpyHostToDevice, nullptr));
    KSP_HIP(hipMemcpy(c->seg_off.p, seg_off, 8 * ((size_t)n_seg + 1), hipMemcpyHostToDevice));
    KSP_HIP(hipMemcpy(c->seg_rec.p, seg_rec, 4 * (size_t)n_seg, hipMemcpyHostToDevice));
    // ---- the hash pass; from here on the batch is counted, and a failure ends the session
    unsigned long long h_count[4] = {0, 0, 0, 0};
    u64 n = 0;
    float ms = 0;
    c->failed = true;
    KSP_HIP(hipEventRecord(ev[0], nullptr));
    if ((rc = classify_launch(c, G, n_bytes, n_seg, true, &n, h_count))) return rc;
    c->st.bases += h_count[1]; c->st.valid_kmers += h_count[2]; c->st.kept_windows += h_count[3];
    if (n > c->hit_cap - c->held) {
        if (c->held) {   // first what is held, sorted and made unique
            u64 left = 0;
            if ((rc = sort_unique_words(who, c->d_hits, c->held, &left))) return rc;
            c->held = left;
            ++c->st.compactions;
        }
        if (n > c->hit_cap - c->held) {   // then the room itself, to the counted need
            const u64 want = c->held + n;
            u64* grown = nullptr;
            if ((rc = ksp::device_fits(who, 8 * want, "8 per hit word held and of this batch"))) return rc;
            KSP_HIP(hipMalloc(&grown, (size_t)want * 8));
            if (c->held && hipMemcpy(grown, c->d_hits, (size_t)c->held * 8, hipMemcpyDeviceToDevice) != hipSuccess) {
                (void)hipFree(grown);
                ksp::set_error(std::string(who) + ": the hit words could not be moved");
                return KSP_E_HIP;
            }
            (void)hipFree(c->d_hits);
            c->d_hits = grown;
            c->hit_cap = want;
        }
        u64 again = 0;
        if ((rc = classify_launch(c, G, n_bytes, n_seg, false, &again, h_count))) return rc;
        if (again != n) { ksp::set_error(std::string(who) + ": the second run of a batch found other hit words than the first"); return KSP_E_HIP; }
        ++c->st.retries;
    }
    KSP_HIP(hipEventRecord(ev[1], nullptr));
    KSP_HIP(hipEventSynchronize(ev[1]));
    KSP_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
    c->held += n;
    c->n_seen = n_seen;
    c->st.hit_words += n;
    c->st.ms_hash += ms;
    ++c->st.batches;
    c->failed = false;
    return KSP_OK;
}

int classify_finish(const char* who, ksp_classify* c, const u32 n_records, const u32 min_hits, ksp_classify_row** rows, u64* n_rows, u32* kept_windows, u32* matched,
                    u32* n_refs_hit, u32* best_ref, u32* best_hits, u32* second_hits, ksp_classify_stats* stats) {
    int rc = KSP_OK;
    if (!c) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    if ((rc = ksp::check_classify_out(who, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits))) return rc;
    if (c->finished || c->failed) { ksp::set_error(std::string(who) + (c->failed ? ": the session has failed" : ": the session is finished")); return KSP_E_ARG; }
    if (c->n_seen > n_records) { ksp::set_error(std::string(who) + ": n_records is not above every record id that was added"); return KSP_E_ARG; }
    if ((rc = ksp::set_device(who, c->device))) return rc;
    ksp::WorkgroupCap G;
    if ((rc = ksp::workgroup_cap("KSPIDER_SKETCH_MAX_WGS", who, G))) return rc;
    ksp::DeviceArena A;
    ksp::Events<2> ev;
    if ((rc = ev.create())) return rc;
    KSP_HIP(hipEventRecord(ev[0], nullptr));
    ksp_classify_row* h_rows = nullptr;
    u64 n_words = 0, n_pairs = 0, n_runs = 0, n_out = 0;
    // the per-record arrays: 5 x 4 per record
    u32 *d_matched = nullptr, *d_refs = nullptr, *d_best_ref = nullptr, *d_best = nullptr, *d_second = nullptr;
    if ((rc = ksp::device_fits(who, 20ull * ((u64)n_records + 1), "20 per record"))) return rc;
    if ((rc = A.alloc(&d_matched, (size_t)n_records + 1)) || (rc = A.alloc(&d_refs, (size_t)n_records + 1)) || (rc = A.alloc(&d_best_ref, (size_t)n_records + 1)) ||
        (rc = A.alloc(&d_best, (size_t)n_records + 1)) || (rc = A.alloc(&d_second, (size_t)n_records + 1)))
        return rc;
    KSP_HIP(hipMemset(d_matched, 0, ((size_t)n_records + 1) * 4));
    u64 *d_scan = nullptr, *d_pairs = nullptr, *d_sorted = nullptr, *d_run = nullptr, *d_n = nullptr;
    u32* d_hits_of = nullptr;
    ksp_classify_row* d_rows = nullptr;
    if (c->held) {
        // ---- the distinct words, and how many pairs they stand for
        if ((rc = sort_unique_words(who, c->d_hits, c->held, &n_words))) return rc;
        c->held = n_words;
        size_t tb = 0, b = 0;
        void* d_tmp = nullptr;
        KSP_HIP(rocprim::exclusive_scan(nullptr, tb, holder_counts_of(nullptr, nullptr, 0), (u64*)nullptr, (u64)0, (size_t)n_words + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        tb = std::max<size_t>(tb, 8);
        if ((rc = ksp::device_fits(who, 8 * (n_words + 1) + tb, "8 per distinct hit word and the scan's scratch"))) return rc;
        if ((rc = A.alloc(&d_scan, (size_t)n_words + 1)) || (rc = A.alloc_bytes(&d_tmp, tb))) return rc;
        hipLaunchKernelGGL(k_classify_matched, dim3(G.grid_of((n_words + 255) / 256)), dim3(256), 0, nullptr, (const u64*)c->d_hits, n_words, d_matched);
        KSP_HIP(hipGetLastError());
        b = tb;
        KSP_HIP(rocprim::exclusive_scan(d_tmp, b, holder_counts_of(c->d_hits, c->T.toff, n_words), d_scan, (u64)0, (size_t)n_words + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        KSP_HIP(hipMemcpy(&n_pairs, d_scan + n_words, 8, hipMemcpyDeviceToHost));
        if (n_pairs < n_words) { ksp::set_error(std::string(who) + ": a hit word without a holder"); return KSP_E_HIP; }
        KSP_HIP(A.release(d_tmp));
        d_tmp = nullptr;
        // ---- the pairs, sorted, and their run lengths
        size_t tb_sort = 0, tb_rle = 0, tb_rows = 0;
        KSP_HIP(rocprim::radix_sort_keys(nullptr, tb_sort, (const u64*)nullptr, (u64*)nullptr, (size_t)n_pairs, 0, 64, (hipStream_t) nullptr));
        KSP_HIP(rocprim::run_length_encode(nullptr, tb_rle, (const u64*)nullptr, (unsigned int)n_pairs, (u64*)nullptr, (u32*)nullptr, (u64*)nullptr, (hipStream_t) nullptr));
        KSP_HIP(rocprim::exclusive_scan(nullptr, tb_rows, row_flags_of(nullptr, 0, 1), (u64*)nullptr, (u64)0, (size_t)n_pairs + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        tb = std::max<size_t>(std::max(std::max(tb_sort, tb_rle), tb_rows), 8);
        if (n_pairs >= (1ull << 32)) { ksp::set_error(std::string(who) + ": 2^32 (record, reference) pairs or more"); return KSP_E_LIMIT; }
        if ((rc = ksp::device_fits(who, 28 * n_pairs + tb + 24, "per (record, reference) hit 8 unsorted, 8 sorted, 8 of the run and 4 of its length, and the sort's scratch"))) return rc;
        if ((rc = A.alloc(&d_pairs, (size_t)n_pairs + 1)) ||   // (+ 1: it later takes the scan of the runs, one value more than there are runs)
(rc = A.alloc(&d_sorted, (size_t)n_pairs)) || (rc = A.alloc(&d_run, (size_t)n_pairs)) ||
            (rc = A.alloc(&d_hits_of, (size_t)n_pairs)) || (rc = A.alloc(&d_n, 1)) || (rc = A.alloc_bytes(&d_tmp, tb)))
            return rc;
        hipLaunchKernelGGL(k_classify_expand, dim3(G.grid_of((n_pairs + 255) / 256)), dim3(256), 0, nullptr, (const u64*)c->d_hits, (const u64*)d_scan, n_words, c->T.toff, c->T.tq,
                           n_pairs, d_pairs);
        KSP_HIP(hipGetLastError());
        b = tb;
        KSP_HIP(rocprim::radix_sort_keys(d_tmp, b, (const u64*)d_pairs, d_sorted, (size_t)n_pairs, 0, 64, (hipStream_t) nullptr));
        b = tb;
        KSP_HIP(rocprim::run_length_encode(d_tmp, b, (const u64*)d_sorted, (unsigned int)n_pairs, d_run, d_hits_of, d_n, (hipStream_t) nullptr));
        KSP_HIP(hipMemcpy(&n_runs, d_n, 8, hipMemcpyDeviceToHost));
        if (n_runs == 0 || n_runs > n_pairs) { ksp::set_error(std::string(who) + ": the run lengths lost their pairs"); return KSP_E_HIP; }
        // ---- the cut at min_hits: the rows in order (d_pairs is free again: it takes the scan)
        b = tb;
        KSP_HIP(rocprim::exclusive_scan(d_tmp, b, row_flags_of(d_hits_of, n_runs, min_hits), d_pairs, (u64)0, (size_t)n_runs + 1, rocprim::plus<u64>(), (hipStream_t) nullptr));
        KSP_HIP(hipMemcpy(&n_out, d_pairs + n_runs, 8, hipMemcpyDeviceToHost));
        if (n_out > n_runs) { ksp::set_error(std::string(who) + ": more rows than runs"); return KSP_E_HIP; }
        if (n_out) {
            if ((rc = ksp::device_fits(who, 16 * n_out, "16 per row"))) return rc;
            if ((rc = A.alloc(&d_rows, (size_t)n_out))) return rc;
            hipLaunchKernelGGL(k_classify_rows, dim3(G.grid_of((n_runs + 255) / 256)), dim3(256), 0, nullptr, (const u64*)d_run, (const u32*)d_hits_of, (const u64*)d_pairs, n_runs,
                               min_hits, d_rows);
            KSP_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_classify_summary, dim3(G.grid_of(((u64)n_records + 255) / 256)), dim3(256), 0, nullptr, (const u64*)d_run, (const u32*)d_hits_of, n_runs, min_hits, n_records,
                       d_refs, d_best_ref, d_best, d_second);
    KSP_HIP(hipGetLastError());
    // ---- to the host
    h_rows = (ksp_classify_row*)std::malloc((size_t)std::max<u64>(n_out, 1) * sizeof(ksp_classify_row));
    if (!h_rows) { ksp::set_error(std::string(who) + ": out of host memory"); return KSP_E_LIMIT; }
    const auto down = [&](void* dst, const void* src, const size_t bytes) {
        if (!bytes) return true;
        const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) ksp::set_error(std::string(who) + ": hipMemcpy of the results: " + hipGetErrorString(e));
        return e == hipSuccess;
    };
    const size_t nr = (size_t)n_records, have = (size_t)std::min<u64>(c->kept_cap, n_records);
    std::fill(kept_windows, kept_windows + nr, 0u);
    if (!down(h_rows, d_rows, (size_t)n_out * sizeof(ksp_classify_row)) || !down(kept_windows, c->d_kept, have * 4) || !down(matched, d_matched, nr * 4) ||
        !down(n_refs_hit, d_refs, nr * 4) || !down(best_ref, d_best_ref, nr * 4) || !down(best_hits, d_best, nr * 4) || !down(second_hits, d_second, nr * 4)) {
        std::free(h_rows);
        return KSP_E_HIP;
    }
    if (hipEventRecord(ev[1], nullptr) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess || hipEventElapsedTime(&c->st.ms_finish, ev[0], ev[1]) != hipSuccess) {
        std::free(h_rows);
        ksp::set_error(std::string(who) + ": the finish could not be timed");
        return KSP_E_HIP;
    }
    c->st.hit_words_unique = n_words;
    c->st.rows = n_out;
    c->finished = true;
    *rows = h_rows;
    *n_rows = n_out;
    if (stats) *stats = c->st;
    return KSP_OK;
}

}  // namespace

extern "C" int ksp_classify_open(int device, int ksize, uint64_t max_hash, uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs,
                                 ksp_classify** out) {
    return classify_open("ksp_classify_open", device, ksize, max_hash, seed, ref_keys, ref_offsets, n_refs, out);
}

extern "C" int ksp_classify_add(ksp_classify* c, const uint8_t* seq, uint64_t n_bytes, const uint64_t* seg_offsets, const uint32_t* seg_records, uint32_t n_segments) {
    const char* who = "ksp_classify_add";
    if (!seg_records) { ksp::set_error(std::string(who) + ": NULL argument"); return KSP_E_ARG; }
    return classify_add(who, c, seq, n_bytes, seg_offsets, seg_records, n_segments);
}

extern "C" int ksp_classify_finish(ksp_classify* c, uint32_t n_records, uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows, uint32_t* kept_windows, uint32_t* matched,
                                   uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits, ksp_classify_stats* stats) {
    return classify_finish("ksp_classify_finish", c, n_records, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits, stats);
}

extern "C" void ksp_classify_close(ksp_classify* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

extern "C" int ksp_classify_host(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* rec_offsets, uint32_t n_records, int ksize, uint64_t max_hash, uint32_t seed,
                                 const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs, uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows,
                                 uint32_t* kept_windows, uint32_t* matched, uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits,
                                 ksp_classify_stats* stats) {
    const char* who = "ksp_classify_host";
    int rc = KSP_OK;
    if ((rc = ksp::check_classify_out(who, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits))) return rc;
    if ((rc = ksp::check_classify_refs(who, ksize, ref_keys, ref_offsets, n_refs))) return rc;
    if ((rc = ksp::check_classify_batch(who, seq, n_bytes, rec_offsets, nullptr, n_records))) return rc;
    ksp_classify* c = nullptr;
    if ((rc = classify_open(who, device, ksize, max_hash, seed, ref_keys, ref_offsets, n_refs, &c))) return rc;
    if (!(rc = classify_add(who, c, seq, n_bytes, rec_offsets, nullptr, n_records)))
        rc = classify_finish(who, c, n_records, min_hits, rows, n_rows, kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits, stats);
    ksp_classify_close(c);
    return rc;
}
