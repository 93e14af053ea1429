// The multi-device job: a client of the engine (engine.hip) through its public C API.  One host thread and one engine per
// device build the block lists (whole, or in slices that are exchanged and assembled), join their share of the tiles, and
// the first device gathers, sorts and hands out the edges: ksp_pairwise_host* / ksp_pairwise_postings_host*.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/kspider_amd.h"
#include "device_call.h"
#include "engine_internal.h"
#include "host_sync.h"
#include "slice_plan.h"

typedef uint64_t u64;
typedef uint32_t u32;

using namespace ksp;

extern "C" {

// results handed to the caller live in pinned host memory (the device-to-host copy runs at the full link
// rate straight into the buffer the caller gets); ksp_free tells them from malloc'ed blocks by this registry
static std::mutex g_pinned_mu;
static std::set<void*> g_pinned;
static void* alloc_result(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> g(g_pinned_mu);
    g_pinned.insert(p);
    return p;
}
void ksp_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_pinned_mu);
        auto it = g_pinned.find(p);
        if (it != g_pinned.end()) { g_pinned.erase(it); (void)hipHostFree(p); return; }
    }
    std::free(p);
}

// ---- collecting the result: join -> [gather to the first device over xGMI] -> device sort -> pinned host ----
// edges of tiles [t0, t1) of a built engine into a device buffer that grows to the size the join reports
static int join_range_grow(ksp_engine* e, u64 t0, u64 t1, Buf& buf, u64& count, float& ms_join) {
    count = 0;
    if (t0 >= t1) return KSP_OK;
    int rc;
    if (buf.bytes < sizeof(ksp_edge)) {
        const u64 first = std::min<u64>(ksp_engine_edge_bound(e, t0, t1) + 1, 1ull << 26);   // at most 1 GiB to begin with
        if ((rc = buf.ensure(first * sizeof(ksp_edge)))) return rc;
    }
    for (int attempt = 0; attempt < 3; ++attempt) {
        u64 cnt = 0;
        rc = ksp_engine_join(e, t0, t1, buf.as<ksp_edge>(), buf.bytes / sizeof(ksp_edge), &cnt, nullptr);
        if (rc != KSP_OK && rc != KSP_E_OVERFLOW) return rc;
        ksp_stats st;
        if (ksp_engine_get_stats(e, &st)) return KSP_E_HIP;
        ms_join += st.ms_join;
        if (rc == KSP_OK) { count = cnt; return KSP_OK; }
        if ((rc = buf.ensure((cnt + cnt / 16 + 1024) * sizeof(ksp_edge)))) {   // (the count the join reported, plus slack)
            set_error("pairwise_host: the edges of this tile range do not fit in device memory");
            return KSP_E_LIMIT;
        }
    }
    set_error("pairwise_host: edge count kept growing between joins");
    return KSP_E_HIP;
}

__global__ void k_edge_split(const ksp_edge* __restrict__ ed, u64 n, u64* __restrict__ key, u64* __restrict__ val) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const ksp_edge x = ed[i];
        key[i] = ((u64)x.source_1 << 32) | x.source_2;
        val[i] = x.shared;
    }
}
__global__ void k_edge_merge(const u64* __restrict__ key, const u64* __restrict__ val, u64 n, ksp_edge* __restrict__ ed) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        ksp_edge x;
        x.source_1 = (u32)(key[i] >> 32);
        x.source_2 = (u32)key[i];
        x.shared = val[i];
        ed[i] = x;
    }
}
// rows in (source_1, source_2) order — the order the TSV writer emits (the reference's own order is hash-map
// iteration order, src/pairwise.cpp:253) — by one device radix sort over the significant key bits
static int sort_edges_device(ksp_edge* d_edges, u64 n, u32 n_sources) {
    if (n < 2) return KSP_OK;
    Buf k0, k1, v0, v1, tmp;
    int rc = KSP_OK;
    do {
        if ((rc = k0.ensure(n * 8)) || (rc = k1.ensure(n * 8)) || (rc = v0.ensure(n * 8)) || (rc = v1.ensure(n * 8))) break;
        const unsigned grid = (unsigned)std::min<u64>((n + 255) / 256, 1u << 20);
        hipLaunchKernelGGL(k_edge_split, dim3(grid), dim3(256), 0, nullptr, d_edges, n, k0.as<u64>(), v0.as<u64>());
        int sbits = 1;
        while (sbits < 32 && (n_sources >> sbits)) ++sbits;
        size_t tb = 0;
        hipError_t err = rocprim::radix_sort_pairs(nullptr, tb, k0.as<u64>(), k1.as<u64>(), v0.as<u64>(), v1.as<u64>(), (size_t)n, 0, 32 + sbits, (hipStream_t) nullptr);
        if (err == hipSuccess && !(rc = tmp.ensure(tb)))
            err = rocprim::radix_sort_pairs(tmp.p, tb, k0.as<u64>(), k1.as<u64>(), v0.as<u64>(), v1.as<u64>(), (size_t)n, 0, 32 + sbits, (hipStream_t) nullptr);
        if (rc) break;
        if (err != hipSuccess) { set_error(std::string("sort_edges: ") + hipGetErrorString(err)); rc = KSP_E_HIP; break; }
        hipLaunchKernelGGL(k_edge_merge, dim3(grid), dim3(256), 0, nullptr, k1.as<u64>(), v1.as<u64>(), n, d_edges);
        err = hipDeviceSynchronize();
        if (err != hipSuccess) { set_error(std::string("sort_edges: ") + hipGetErrorString(err)); rc = KSP_E_HIP; }
    } while (0);
    k0.release(); k1.release(); v0.release(); v1.release(); tmp.release();
    return rc;
}

}  // extern "C"

// ---- what a job may also want from its edges (AfterJoin, engine_internal.h) ----
// A new consumer is added here and nowhere in the worker: its argument check in after_join_check, its call in after_join_run.
static int after_join_check(const AfterJoin* after) {
    if (!after) return KSP_OK;
    if (after->kind == AfterJoin::kTree && (after->col < 3 || after->col > 5)) { set_error("pairwise: a tree needs a column 3 / 4 / 5 and room for its result"); return KSP_E_ARG; }
    if (after->kind == AfterJoin::kTopk && (after->col < 3 || after->col > 5 || after->k < 1 || after->k > KSP_TOPK_MAX_K)) { set_error("pairwise: top-k needs a column 3 / 4 / 5 and 1 <= k <= KSP_TOPK_MAX_K"); return KSP_E_ARG; }
    if (after->kind == AfterJoin::kReport && (after->col < 3 || after->col > 5 || after->cutoff != after->cutoff)) { set_error("pairwise: a cluster report needs a column 3 / 4 / 5 and a cut-off that is a number"); return KSP_E_ARG; }
    if (after->kind == AfterJoin::kUpgma && (after->col < 3 || after->col > 5)) { set_error("pairwise: an average-linkage tree needs a column 3 / 4 / 5"); return KSP_E_ARG; }
    if (after->kind == AfterJoin::kSweep && (!after->cutoffs || after->n_cutoffs < 1 || after->n_cutoffs > KSP_SWEEP_MAX_CUTOFFS)) {
        set_error("pairwise: a cut-off ladder has between 1 and 255 cut-offs");
        return KSP_E_ARG;
    }
    if (after->want_text && (!after->kmer_counts || !after->ids || !after->text_sink)) { set_error("pairwise: the rows' text needs the k-mer counts, the ids and a sink"); return KSP_E_ARG; }
    return KSP_OK;
}
// the rows' text (AfterJoin::want_text) from the sorted edges on the current device, piece by piece into the job's sink
static int after_join_text(AfterJoin& A, const u32 N, const ksp_edge* d_all, const u64 total) {
    A.text_bytes = 0;
    if (!N || !total) return KSP_OK;
    Buf d_cnt, d_ids;
    u64 n_bytes = 0, handed = 0;
    const TsvSink sink = [&](const char* p, const uint64_t n) { handed += n; return A.text_sink(p, n); };
    int rc;
    if ((rc = d_cnt.ensure((size_t)N * 4)) || (rc = d_ids.ensure((size_t)N * 4)) || (rc = ksp_memcpy_h2d(d_cnt.p, A.kmer_counts, (u64)N * 4)) ||
        (rc = ksp_memcpy_h2d(d_ids.p, A.ids, (u64)N * 4)) ||
        (rc = tsv_edges_on_device("pairwise (KSPIDER_TSV=device)", N, d_all, total, d_cnt.as<u32>(), d_ids.as<u32>(), ~0ull, &sink, &n_bytes))) {}
    else if (handed != n_bytes) { set_error("pairwise (KSPIDER_TSV=device): the pieces do not add up to the text"); rc = KSP_E_HIP; }
    A.text_bytes = handed;
    d_cnt.release(); d_ids.release();
    return rc;
}
// the consumers of the sorted edges (every kind but kNone and kCut, which is applied before the gather), on the current device,
// from HBM: the same edge records, which never travel to the host and back as text for this
static int after_join_run(AfterJoin& A, const u32 N, const ksp_edge* d_all, const u64 total) {
    if (A.kind == AfterJoin::kNone || A.kind == AfterJoin::kCut) return KSP_OK;
    int rc = KSP_OK;
    Buf d_cnt;
    const bool run = N && !(rc = d_cnt.ensure((size_t)N * 4)) && !(rc = ksp_memcpy_h2d(d_cnt.p, A.kmer_counts, (u64)N * 4));
    u32 n_out = 0;   // kRepr: the sources ranked, kTree: the records of the forest
    switch (A.kind) {
        case AfterJoin::kCluster:
            A.labels.assign((size_t)N, 0);
            if (run) rc = cc_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.cutoff, A.labels.data(), &A.n_kept, A.ksize);
            break;
        case AfterJoin::kSweep:   // one classification of the records, components continued from rank to rank
            A.labels.assign((size_t)A.n_cutoffs * N, 0);
            A.kept.assign(A.n_cutoffs, 0);
            if (run) rc = sweep_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.cutoffs, A.n_cutoffs, A.labels.data(), A.kept.data());
            break;
        case AfterJoin::kTree:
            A.index.assign((size_t)std::min<u64>(N ? N - 1 : 0, total) + 1, 0);
            if (run) rc = tree_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.index.data(), &n_out);
            A.index.resize(n_out);
            break;
        case AfterJoin::kDerep:   // (the ranks go to A.node; without a source nothing is asked)
            A.rep.assign((size_t)N, 0); A.via.assign((size_t)N, 0); A.node.assign((size_t)N, 0); A.degree.assign((size_t)N, 0);
            if (run) rc = derep_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.threshold, A.rep.data(), A.via.data(), A.node.data(),
                                                A.degree.data(), &n_out, &A.derep);
            break;
        case AfterJoin::kTopk:   // (index: n_sources x k record indices, count: the hits of every source)
            A.index.assign((size_t)N * A.k, 0xFFFFFFFFu); A.count.assign((size_t)N, 0);
            if (run) rc = topk_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.k, A.index.data(), A.count.data(), &A.topk);
            break;
        case AfterJoin::kReport:   // (cluster_rows: the clusters in root order, member_rows: one row per source)
            A.cluster_rows.assign((size_t)N + 1, ksp_cluster_row()); A.member_rows.assign((size_t)N + 1, ksp_member_row());
            if (run) rc = report_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.cutoff, A.cluster_rows.data(), &n_out, A.member_rows.data(), &A.report);
            A.cluster_rows.resize(n_out); A.member_rows.resize((size_t)N);
            break;
        case AfterJoin::kUpgma:   // (upgma_rows: the merges in merge order)
            A.upgma_rows.assign((size_t)N + 1, ksp_upgma_row());
            if (run) rc = upgma_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.upgma_rows.data(), &n_out, &A.upgma);
            A.upgma_rows.resize(n_out);
            break;
        default:   // kRepr
            A.node.assign((size_t)N, 0);
            A.count.assign((size_t)N, 0);
            if (run) rc = repr_edges_on_device(N, d_all, total, d_cnt.as<u32>(), A.col, A.threshold, nullptr, A.node.data(), A.count.data(), &n_out);
            A.node.resize(n_out);
            A.count.resize(n_out);
    }
    d_cnt.release();
    return rc;
}

// `bytes` from the host into a fresh allocation on `device` (ksp_memcpy_h2d is synchronous: complete on return)
static int upload(const int device, const void* h, const u64 bytes, void** d) {
    const int rc = ksp_device_malloc(device, bytes, d);
    return rc ? rc : ksp_memcpy_h2d(*d, h, bytes);
}

namespace {
struct MultiJob {
    // input (host): sketches (keys / weights / offsets) or an inverted index (key_off / sources / key_weights)
    const u64* keys = nullptr; const u32* weights = nullptr; const u64* offsets = nullptr;
    const u64* key_off = nullptr; const u32* sources = nullptr; const u32* key_weights = nullptr;
    u32 n_keys = 0, n_sources = 0;
    bool postings = false;
    ksp::AfterJoin* after = nullptr;   // what is also wanted from the edges (engine_internal.h)
    bool wants(ksp::AfterJoin::Kind k) const { return after && after->kind == k; }
};

struct Worker;
// what the workers of one job share: the plan, the barrier, and what one worker writes in a step for the others to read in the next
struct MultiRun {
    const MultiJob& job;
    const SlicePlan& plan;
    const int nd;                 // workers: one per slice (there may be several on a device)
    const int* const devices;     // ... and the device of each
    const bool sliced, weighted;
    const u32 N;
    const u64 n;                  // entries / memberships of the input
    FailBarrier bar;              // (the failure decision is latched once per barrier generation: host_sync.h)
    std::vector<Worker> w;
    std::vector<u32> lab_min;     // MIN-combined labels (host)
    std::vector<u32> bnd_sum;     // per-source counter bounds summed over postings slices (host)
    std::vector<u64> all_sizes;   // ksp_engine_slice_sizes of every slice
    u64 total = 0;
    std::vector<u64> edge_off;
    Buf merged;                   // all edges on the first device (nd > 1)
    ksp_edge** out_edges; uint64_t* n_edges; ksp_stats* stats;
    MultiRun(const MultiJob& j, const SlicePlan& p, u64 n_, ksp_edge** oe, uint64_t* ne, ksp_stats* st);
};

// One device thread of the job.  Its steps are the rows of kSteps below, in that order; run() is the only caller.  A step returns
// a KSP_* code and has left its text in ksp_last_error(); what it allocated is released by run_multi whatever happened.
struct Worker {
    MultiRun* R = nullptr;
    int i = 0, device = 0;
    ksp_engine* e = nullptr;
    void *d_a = nullptr, *d_b = nullptr;      // keys + weights, or sources + key weights
    int owner = 0;                            // the first worker on my device uploads the input; the others use its copy
    bool borrowed = false;                    // d_a / d_b belong to another worker on the same device
    std::vector<u64> my_off;                  // postings slices: key offsets of my slice, from 0
    u32 my_keys = 0;
    Buf edges, labels, gather[6], exp[6];
    std::vector<u32> lab, bnd;                // my slice's labels and counter bounds (host)
    u64 sizes[4] = {0, 0, 0, 0};
    u64 lstride = 4, bigstride = 1;           // every device receives every slice: [part][stride] buffers, filled by peer copies from the owners
    size_t bytes[6] = {0, 0, 0, 0, 0, 0};
    std::vector<u64> cuts;
    u64 n_block_keys = 0, last_tiles = 0, last_pairs = 0;   // ksp_stats of my engine after its build / its join
    u64 count = 0, found = 0;                 // count: edges I hand on; found: edges of my join (the same without a cut)
    float ms_join = 0;
    int failed = KSP_OK;                      // the code and the text of the step that failed here
    std::string error;

    int upload_input() {
        const MultiJob& job = R->job;
        int rc = ksp_engine_create(device, &e);
        if (rc) return rc;
        for (int j = 0; j < R->nd; ++j)   // direct xGMI copies between the devices of this job (already enabled: fine)
            if (R->devices[j] != device) { (void)hipDeviceEnablePeerAccess(R->devices[j], 0); (void)hipGetLastError(); }
        const void *h_a, *h_b;
        u64 bytes_a, bytes_b;
        if (job.postings && R->sliced) {   // every worker uploads its own slice of the index
            const u32 k0 = R->plan.pk_cut[(size_t)i], k1 = R->plan.pk_cut[(size_t)i + 1];
            my_keys = k1 - k0;
            my_off.resize((size_t)my_keys + 1);
            const u64 e0 = job.key_off[k0];
            for (u32 k = 0; k <= my_keys; ++k) my_off[k] = job.key_off[k0 + k] - e0;
            h_a = job.sources + e0; bytes_a = my_off[my_keys] * 4;
            // (allocated even for an empty slice: a non-NULL weight array is what makes a build weighted)
            h_b = job.key_weights ? job.key_weights + k0 : nullptr; bytes_b = (u64)my_keys * 4;
        } else {
            for (int j = 0; j < i; ++j)
                if (R->devices[j] == device) { owner = j; break; }
            if (!R->n || owner != i) return KSP_OK;
            if (job.postings) { h_a = job.sources; bytes_a = R->n * 4; h_b = job.key_weights; bytes_b = (u64)job.n_keys * 4; }
            else { h_a = job.keys; bytes_a = R->n * 8; h_b = job.weights; bytes_b = R->n * 4; }
        }
        if ((rc = upload(device, h_a, bytes_a, &d_a))) return rc;
        return h_b ? upload(device, h_b, bytes_b, &d_b) : KSP_OK;
    }
    int build_slice() {
        const MultiJob& job = R->job;
        if (owner != i) { d_a = R->w[(size_t)owner].d_a; d_b = R->w[(size_t)owner].d_b; borrowed = true; }
        if (job.postings && R->sliced) return ksp_engine_build_postings_slice(e, my_off.data(), (const u32*)d_a, (const u32*)d_b, my_keys, R->N, nullptr);
        if (job.postings) return ksp_engine_build_postings(e, job.key_off, (const u32*)d_a, (const u32*)d_b, job.n_keys, R->N, nullptr);
        if (R->nd == 1) return ksp_engine_build_blocks(e, (const u64*)d_a, (const u32*)d_b, job.offsets, R->N, 0, nullptr);
        return ksp_engine_build_slice(e, (const u64*)d_a, (const u32*)d_b, job.offsets, R->N, 0, (u32)i, (u32)R->nd, nullptr);
    }
    int read_labels_and_bounds() {
        const u32 N = R->N;
        if (!N) return KSP_OK;
        int rc;
        lab.resize(N);   // common source order: element-wise MIN of the devices' labels
        if ((rc = labels.ensure((size_t)N * 4)) || (rc = ksp_engine_slice_labels(e, labels.as<u32>(), nullptr)) ||
            (rc = ksp_memcpy_d2h(lab.data(), labels.p, (u64)N * 4)))
            return rc;
        if (!R->job.postings) return KSP_OK;
        bnd.resize(N);   // postings slices hold a share of every source's keys: the counters' bounds are the sums over the slices
        if ((rc = ksp_engine_slice_bounds(e, labels.as<u32>(), nullptr))) return rc;
        return ksp_memcpy_d2h(bnd.data(), labels.p, (u64)N * 4);
    }
    int combine_on_first() {
        if (i != 0) return KSP_OK;
        const u32 N = R->N;
        R->lab_min = lab;
        for (int j = 1; j < R->nd; ++j)
            for (u32 s = 0; s < N; ++s) R->lab_min[s] = std::min(R->lab_min[s], R->w[(size_t)j].lab[s]);
        if (R->job.postings && N) {
            R->bnd_sum.assign(N, 0);
            for (int j = 0; j < R->nd; ++j)
                for (u32 s = 0; s < N; ++s) R->bnd_sum[s] = (u32)std::min<u64>((u64)R->bnd_sum[s] + R->w[(size_t)j].bnd[s], 0xFFFFFFFFull);
        }
        return KSP_OK;
    }
    int finish_slice() {
        const u32 N = R->N;
        int rc;
        if (N && R->job.postings &&
            ((rc = ksp_memcpy_h2d(labels.p, R->bnd_sum.data(), (u64)N * 4)) || (rc = ksp_engine_slice_set_bounds(e, labels.as<u32>(), nullptr))))
            return rc;
        if (N && ((rc = ksp_memcpy_h2d(labels.p, R->lab_min.data(), (u64)N * 4)) || (rc = ksp_engine_slice_finish(e, labels.as<u32>(), nullptr)))) return rc;
        if (!N && (rc = ksp_engine_slice_finish(e, nullptr, nullptr))) return rc;
        if ((rc = ksp_engine_slice_sizes(e, sizes))) return rc;
        for (int q = 0; q < 4; ++q) R->all_sizes[(size_t)i * 4 + q] = sizes[q];
        return KSP_OK;
    }
    int export_slice() {
        const int nd = R->nd;
        for (int j = 0; j < nd; ++j) { lstride = std::max(lstride, R->all_sizes[(size_t)j * 4]); bigstride = std::max(bigstride, R->all_sizes[(size_t)j * 4 + 2]); }
        ksp_stats st;
        int rc = ksp_engine_get_stats(e, &st);
        if (rc) return rc;
        const size_t nb = (size_t)st.n_blocks;   // (the same on every device: a function of the source count; set when the build begins)
        bytes[0] = bytes[1] = lstride * 4; bytes[2] = R->weighted ? lstride * 4 : 0; bytes[3] = bytes[4] = (nb + 1) * 4; bytes[5] = bigstride * 16;
        for (int q = 0; q < 6; ++q) {
            if (!bytes[q]) continue;
            if ((rc = exp[q].ensure(bytes[q])) || (rc = gather[q].ensure(bytes[q] * (size_t)nd))) return rc;
            if (hipMemset(exp[q].p, 0, bytes[q]) != hipSuccess || hipMemset(gather[q].p, 0, bytes[q] * (size_t)nd) != hipSuccess) { set_error("pairwise: hipMemset"); return KSP_E_HIP; }
        }
        if (!R->n) return KSP_OK;
        return ksp_engine_slice_export(e, exp[0].as<u32>(), exp[1].as<u32>(), R->weighted ? exp[2].as<u32>() : nullptr, exp[3].as<u32>(), exp[4].as<u32>(),
                                       exp[5].p, nullptr);
    }
    int send_slices() {
        for (int j = 0; j < R->nd && !R->bar.failed_hint(); ++j)      // my slice into device j's gather buffers
            for (int q = 0; q < 6; ++q) {
                if (!bytes[q]) continue;
                if (hipMemcpyPeer((char*)R->w[(size_t)j].gather[q].p + bytes[q] * (size_t)i, R->devices[j], exp[q].p, device, bytes[q]) != hipSuccess) {
                    set_error("pairwise: peer copy of a block-list slice failed");
                    return KSP_E_HIP;
                }
            }
        return KSP_OK;
    }
    int assemble() {
        return ksp_engine_assemble(e, (u32)R->nd, R->all_sizes.data(), gather[0].as<u32>(), gather[1].as<u32>(), R->weighted ? gather[2].as<u32>() : nullptr,
                                   lstride, gather[3].as<u32>(), gather[4].as<u32>(), gather[5].p, bigstride, nullptr);
    }
    int tile_cuts() {
        cuts.assign((size_t)R->nd + 1, 0);
        int rc;
        ksp_stats st;
        if ((rc = ksp_engine_balanced_cuts(e, (u32)R->nd, cuts.data())) || (rc = ksp_engine_get_stats(e, &st))) return rc;
        n_block_keys = st.n_block_keys;
        return KSP_OK;
    }
    int check_cuts_on_first() {
        if (i != 0) return KSP_OK;
        for (int j = 1; j < R->nd; ++j)
            if (R->w[(size_t)j].cuts != cuts || R->w[(size_t)j].n_block_keys != n_block_keys) {
                set_error("pairwise: the devices built different block lists (cannot shard the tiles)");
                return KSP_E_HIP;
            }
        return KSP_OK;
    }
    int join_and_cut() {
        int rc;
        if ((rc = join_range_grow(e, cuts[(size_t)i], cuts[(size_t)i + 1], edges, count, ms_join))) return rc;
        ksp_stats st;
        if ((rc = ksp_engine_get_stats(e, &st))) return rc;
        last_tiles = st.last_tiles; last_pairs = st.last_pairs;
        found = count;
        AfterJoin* const after = R->job.after;
        if (R->job.wants(AfterJoin::kCut) && count) {   // the cut, on my own edges: what follows (gather, sort, copy) sees the kept records only
            Buf d_cnt, kept;
            CutPass pass;
            u64 n_kept = 0;
            if ((rc = d_cnt.ensure((size_t)R->N * 4)) || (rc = ksp_memcpy_h2d(d_cnt.p, after->kmer_counts, (u64)R->N * 4)) ||
                (rc = cut_count_on_device(edges.as<ksp_edge>(), count, d_cnt.as<u32>(), after->col, after->cutoff, pass, &n_kept))) {}
            else if (n_kept == count) {}   // (every record passes: they stay where they are)
            else if (n_kept == 0) count = 0;
            else if ((rc = kept.ensure(n_kept * sizeof(ksp_edge))) ||   // (sized by the count pass's total, not by the input)
                     (rc = cut_scatter_on_device(edges.as<ksp_edge>(), count, d_cnt.as<u32>(), after->col, pass, kept.as<ksp_edge>()))) {}
            else {
                edges.release();
                edges = kept;
                kept = Buf();
                count = n_kept;
            }
            pass.release(); d_cnt.release(); kept.release();
        }
        return rc;
    }
    int place_edges_on_first() {
        if (i != 0) return KSP_OK;
        const int nd = R->nd;
        for (int j = 0; j < nd; ++j) R->edge_off[(size_t)j + 1] = R->edge_off[(size_t)j] + R->w[(size_t)j].count;
        R->total = R->edge_off[(size_t)nd];
        if (R->job.wants(AfterJoin::kCut))
            for (int j = 0; j < nd; ++j) R->job.after->n_found += R->w[(size_t)j].found;
        return nd > 1 && R->total ? R->merged.ensure(R->total * sizeof(ksp_edge)) : KSP_OK;
    }
    int gather_edges() {
        if (R->nd > 1 && count &&      // the gather to the first device: one peer copy per device (xGMI)
            hipMemcpyPeer((char*)R->merged.p + R->edge_off[(size_t)i] * sizeof(ksp_edge), R->devices[0], edges.p, device, count * sizeof(ksp_edge)) != hipSuccess) {
            set_error("pairwise: peer copy of the edges failed");
            return KSP_E_HIP;
        }
        return KSP_OK;
    }
    int collect_on_first() {
        if (i != 0) return KSP_OK;
        const u64 total = R->total;
        ksp_edge* d_all = R->nd > 1 ? R->merged.as<ksp_edge>() : edges.as<ksp_edge>();
        int rc;
        if (total && (rc = sort_edges_device(d_all, total, R->N))) return rc;
        if (R->job.after && (rc = after_join_run(*R->job.after, R->N, d_all, total))) return rc;
        bool skip_copy = false;   // the device wrote the rows and no finisher reads the records: they stay where they are
        if (AfterJoin* const after = R->job.after; after && after->want_text) {
            if ((rc = after_join_text(*after, R->N, d_all, total))) return rc;
            skip_copy = after->edges_skipped = after->kind == AfterJoin::kNone || after->kind == AfterJoin::kCut;
        }
        ksp_edge* out = (ksp_edge*)alloc_result(skip_copy ? 0 : total * sizeof(ksp_edge));
        if (!out) { set_error("pairwise_host: out of pinned host memory"); return KSP_E_LIMIT; }
        if (total && !skip_copy && (rc = ksp_memcpy_d2h(out, d_all, total * sizeof(ksp_edge)))) { ksp_free(out); return rc; }
        *R->out_edges = out;
        *R->n_edges = total;
        if (ksp_stats* stats = R->stats) {
            ksp_engine_get_stats(e, stats);
            stats->ms_join = 0; stats->last_tiles = 0; stats->last_pairs = 0;
            for (const Worker& W : R->w) {
                stats->ms_join = std::max(stats->ms_join, W.ms_join);
                stats->last_tiles += W.last_tiles;
                stats->last_pairs += W.last_pairs;
            }
            stats->last_edges = total;
        }
        return KSP_OK;
    }
    void run();
};

MultiRun::MultiRun(const MultiJob& j, const SlicePlan& p, u64 n_, ksp_edge** oe, uint64_t* ne, ksp_stats* st)
    : job(j), plan(p), nd((int)p.devices.size()), devices(p.devices.data()), sliced(p.sliced),
      weighted(j.postings ? j.key_weights != nullptr : j.weights != nullptr), N(j.n_sources), n(n_), bar(nd), all_sizes((size_t)nd * 4, 0),
      edge_off((size_t)nd + 1, 0), out_edges(oe), n_edges(ne), stats(st) {}

// The job, step by step.  Every worker passes the same sequence of barriers whatever failed and wherever: a step is skipped
// when a failure is already known, the barrier behind it never, and the steps of the sliced path are skipped by all workers or
// by none (`sliced` is job-wide).  A step that reads what another worker wrote does so in a later row than the write.
// host_sync_check.cpp checks this loop's skeleton with as many stages (ksp::kMultiSteps, host_sync.h).
struct Step {
    int (Worker::*fn)();
    bool sliced_only;
};
const Step kSteps[] = {
    {&Worker::upload_input, false},             // stage 1: an engine, and my share of the input in its HBM
    {&Worker::build_slice, false},              //   my slice, or the whole input
    {&Worker::read_labels_and_bounds, true},    //   the slices become the full lists on every device: MIN of the labels and
    {&Worker::combine_on_first, true},          //   saturating sum of the bounds, then every slice to every device
    {&Worker::finish_slice, true},
    {&Worker::export_slice, true},
    {&Worker::send_slices, true},
    {&Worker::assemble, true},
    {&Worker::tile_cuts, false},                // stage 2: my share of the tiles
    {&Worker::check_cuts_on_first, false},
    {&Worker::join_and_cut, false},
    {&Worker::place_edges_on_first, false},
    {&Worker::gather_edges, false},
    {&Worker::collect_on_first, false},         //   sort, the after-join consumer, the result
};
static_assert(sizeof kSteps / sizeof kSteps[0] == kMultiSteps, "host_sync_check.cpp checks the barrier loop with kMultiSteps stages");

void Worker::run() {
    for (const Step& s : kSteps) {
        if (s.sliced_only && !R->sliced) continue;
        if (!R->bar.failed_hint()) {
            const int step_rc = (this->*s.fn)();
            if (step_rc) { failed = step_rc; error = ksp_last_error(); R->bar.fail(); }
        }
        if (R->bar.sync()) return;
    }
}
}  // namespace

// The whole job on `nd` devices, one host thread + one engine per device (the reference entry points call this
// with the devices of $KSPIDER_DEVICES; nd = 1 is the single-GPU path):
//   stage 1   device i builds its slice — sketch input: its 1/nd share of the hash range; postings input (the reference's
//             entry point): 1/nd of the colours (whole keys, cut by memberships) — the labels are MIN-combined and the
//             slices exchanged device to device (peer copies over xGMI), then every device assembles the full lists:
//             the same exchange kspider_amd/dist.py does with RCCL collectives between processes.  Inputs of 2^30
//             entries or more are cut into more slices than there are devices (several workers per device: slice_plan.h).
//   stage 2   device i joins the tile range [cuts[i], cuts[i+1]) of equal estimated work (same cuts everywhere:
//             checked), the edges are gathered to the first device (peer copies), sorted there and copied into
//             pinned host memory.
static int run_multi(const MultiJob& job, const int* devices, int nd, ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats) {
    *out_edges = nullptr;
    *n_edges = 0;
    if (nd < 1 || nd > 64) { set_error("pairwise: between 1 and 64 devices"); return KSP_E_ARG; }
    int rc = after_join_check(job.after);
    if (rc) return rc;
    if (job.after) job.after->n_found = 0;
    const u64 n = job.postings ? (job.n_keys ? job.key_off[job.n_keys] : 0) : (job.n_sources ? job.offsets[job.n_sources] : 0);
    SlicePlan plan;
    if ((rc = plan_slices(job.postings, n, job.n_keys, job.key_off, devices, nd, std::getenv("KSP_SLICES"), plan))) return rc;
    MultiRun R(job, plan, n, out_edges, n_edges, stats);
    nd = R.nd;
    R.w.resize((size_t)nd);
    for (int i = 0; i < nd; ++i) { Worker& W = R.w[(size_t)i]; W.R = &R; W.i = W.owner = i; W.device = R.devices[i]; }
    if (nd == 1) R.w[0].run();
    else {
        std::vector<std::thread> th;
        for (int i = 0; i < nd; ++i) th.emplace_back(&Worker::run, &R.w[(size_t)i]);
        for (auto& t : th) t.join();
    }
    for (int i = 0; i < nd; ++i) {
        Worker& W = R.w[(size_t)i];
        if (W.failed && !rc) { rc = W.failed; set_error(W.error); }   // (the lowest-numbered worker that failed)
        if (W.e) (void)hipSetDevice(W.device);
        if (W.d_a && !W.borrowed) (void)hipFree(W.d_a);
        if (W.d_b && !W.borrowed) (void)hipFree(W.d_b);
        W.edges.release(); W.labels.release();
        for (int q = 0; q < 6; ++q) { W.gather[q].release(); W.exp[q].release(); }
        ksp_engine_destroy(W.e);
    }
    if (nd > 1 || R.merged.p) { (void)hipSetDevice(R.devices[0]); R.merged.release(); }
    if (rc && *out_edges) { ksp_free(*out_edges); *out_edges = nullptr; *n_edges = 0; }
    return rc;
}

int ksp::pairwise_postings_multi_cc(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights, uint32_t n_keys,
                                    uint32_t n_sources, const int* devices, int n_devices, ksp_edge** out_edges, uint64_t* n_edges,
                                    ksp_stats* stats, AfterJoin* after) {
    if (!out_edges || !n_edges || !devices || (n_keys && (!key_off || !sources))) { set_error("pairwise_postings_host: NULL argument"); return KSP_E_ARG; }
    const u64 n = n_keys ? key_off[n_keys] : 0;
    for (u64 i = 0; i < n; ++i)
        if (sources[i] >= n_sources) { set_error("pairwise_postings_host: source index out of range"); return KSP_E_ARG; }
    MultiJob job;
    job.postings = true;
    job.key_off = key_off; job.sources = sources; job.key_weights = key_weights; job.n_keys = n_keys; job.n_sources = n_sources;
    job.after = after;
    return run_multi(job, devices, n_devices, out_edges, n_edges, stats);
}
extern "C" {

int ksp_pairwise_host_multi(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                            const int* devices, int n_devices, ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats) {
    if (!offsets || !out_edges || !n_edges || !devices) { set_error("pairwise_host: NULL argument"); return KSP_E_ARG; }
    MultiJob job;
    job.keys = keys; job.weights = weights; job.offsets = offsets; job.n_sources = n_sources;
    return run_multi(job, devices, n_devices, out_edges, n_edges, stats);
}

int ksp_pairwise_host_cut(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                          const uint32_t* kmer_counts, int dist_col, double cutoff, const int* devices, int n_devices,
                          ksp_edge** out_edges, uint64_t* n_edges, uint64_t* n_found, ksp_stats* stats) {
    if (!offsets || !out_edges || !n_edges || !devices) { set_error("ksp_pairwise_host_cut: NULL argument"); return KSP_E_ARG; }
    if (dist_col < 3 || dist_col > 5) { set_error("ksp_pairwise_host_cut: dist_col is 3 (min), 4 (avg) or 5 (max containment)"); return KSP_E_ARG; }
    if (cutoff != cutoff) { set_error("ksp_pairwise_host_cut: the cut-off is NaN"); return KSP_E_ARG; }
    std::vector<u32> lengths;
    if (!kmer_counts) {   // the k-mer count of a source is the length of its run
        lengths.resize(n_sources);
        for (u32 v = 0; v < n_sources; ++v) {
            const u64 len = offsets[v + 1] - offsets[v];
            if (len > 0xFFFFFFFFull) { set_error("ksp_pairwise_host_cut: a run of 2^32 keys or more"); return KSP_E_LIMIT; }
            lengths[v] = (u32)len;
        }
        kmer_counts = lengths.data();
    }
    AfterJoin cut;
    cut.kind = AfterJoin::kCut; cut.kmer_counts = kmer_counts; cut.col = dist_col; cut.cutoff = cutoff;
    MultiJob job;
    job.keys = keys; job.weights = weights; job.offsets = offsets; job.n_sources = n_sources;
    job.after = &cut;
    if (n_found) *n_found = 0;
    const int rc = run_multi(job, devices, n_devices, out_edges, n_edges, stats);
    if (!rc && n_found) *n_found = cut.n_found;
    return rc;
}

int ksp_pairwise_postings_host_multi(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights,
                                     uint32_t n_keys, uint32_t n_sources, const int* devices, int n_devices,
                                     ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats) {
    return ksp::pairwise_postings_multi_cc(key_off, sources, key_weights, n_keys, n_sources, devices, n_devices, out_edges, n_edges, stats, nullptr);
}

int ksp_pairwise_host(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                      int device, ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats) {
    return ksp_pairwise_host_multi(keys, weights, offsets, n_sources, &device, 1, out_edges, n_edges, stats);
}

int ksp_pairwise_postings_host(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights,
                               uint32_t n_keys, uint32_t n_sources, int device, ksp_edge** out_edges,
                               uint64_t* n_edges, ksp_stats* stats) {
    return ksp_pairwise_postings_host_multi(key_off, sources, key_weights, n_keys, n_sources, &device, 1, out_edges, n_edges, stats);
}

}  // extern "C"
