/* kspider_amd — C ABI of the MI355X-native pairwise containment engine.
 *
 * This is the drop-in boundary for ONE path of dib-lab/kSpider: kSpider::pairwise()
 * (reference: include/kSpider.hpp:11, src/pairwise.cpp:123-276, SWIG wrapper
 * src/swig_interfaces/kSpider_internal.i:11).  Plain pointers and sizes only; no
 * torch / C++ types.  Every function returns 0 on success, a KSP_E_* code otherwise;
 * ksp_last_error() gives the message of the calling thread's last failure.
 *
 * There is NO CPU fallback behind these entry points: without a visible gfx950
 * device (or without the HIP runtime) they fail with KSP_E_HIP.
 */
#ifndef KSPIDER_AMD_H
#define KSPIDER_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    KSP_OK = 0,
    KSP_E_ARG = 1,      /* bad argument */
    KSP_E_HIP = 2,      /* HIP runtime / device failure */
    KSP_E_IO = 3,       /* missing / malformed index file */
    KSP_E_OVERFLOW = 4, /* edge buffer too small: *count holds the required size */
    KSP_E_LIMIT = 5     /* input exceeds an engine limit */
};

/* One row of the reference's PAIRS_COUNTER (src/pairwise.cpp:22-27):
 * key pair<uint32,uint32> with source_1 < source_2, value uint64 shared k-mers. */
typedef struct ksp_edge {
    uint32_t source_1;
    uint32_t source_2;
    uint64_t shared;
} ksp_edge;

typedef struct ksp_engine ksp_engine;

typedef struct ksp_stats {
    uint64_t n_sources;
    uint64_t n_entries;     /* sum of sketch sizes                                  */
    uint64_t n_blocks;      /* blocks of 128 source slots: ceil(n_sources / 128), or up to half as many again when the
                               source reordering keeps clusters inside blocks (slots without a source stay empty) */
    uint64_t n_block_keys;  /* distinct keys summed over blocks                     */
    uint64_t n_tiles;       /* n_blocks (n_blocks + 1) / 2                          */
    uint64_t last_tiles;    /* tiles joined by the last ksp_engine_join             */
    uint64_t last_pairs;    /* source pairs covered by the last ksp_engine_join     */
    uint64_t last_stream_bytes; /* bytes the join kernel streamed (model) */
    uint64_t last_edges;    /* non-zero pairs found by the last join                */
    float ms_build;         /* HIP-event time of the last build_blocks (all kernels) */
    float ms_join;          /* HIP-event time of the last join kernel launch        */
    int weighted;
    int key_bits;
    uint64_t n_active_tiles;    /* tiles with something to count (block pairs sharing a key, diagonal
                                   tiles of blocks with a multi-source key); = n_tiles in dense mode */
    uint64_t last_active_tiles; /* ... among the tiles of the last ksp_engine_join                   */
    uint64_t sort_entries;      /* entries of the global radix sort of the last build (rocPRIM onesweep:
                                   8-byte key + 4/8-byte tag read and written once per 8-bit pass)      */
    float ms_sort;              /* its HIP-event time (all passes + histogram)                        */
    int sort_bits;              /* key bits it sorted on                                              */
    int partition_kind;         /* how the last build brought equal keys together: 0 nothing to do / postings
                                   input, 1 rocPRIM radix partition or sort, 2 the hand-written paged
                                   partition, 3 the segment partition: level 1 read off the sorted runs
                                   (partition_kernels.hip.h)                                             */
    int partition_fallback;     /* 0, or why a hand-written partition handed the last build on: 1 page table / pool
                                   full (keys far from uniform; -> rocPRIM), 2 internal count mismatch, 3 page
                                   wait timed out (2 and 3 are defects, never expected), 4 / 5 a tile / a bucket
                                   of the segment partition overflowed (-> the paged partition).  Such a hand-over
                                   sticks to the engine: its later builds go straight to the fallback and report 0 */
    uint64_t n_match_records;   /* match-list join: (key, block pair) records stage 1 handed to the join (0: the
                                   join searches the block lists)                                         */
    uint64_t n_join_workgroups; /* shares of the work list (workgroups of a join over all tiles)           */
    uint64_t n_kept_entries;    /* entries whose key is held by at least two sources (the others are pruned) */
    uint64_t n_kept_keys;       /* distinct keys among them                                                */
    int stage1_kind;            /* middle of stage 1: 1 bucket-resident (grouping + emit + labels in one kernel, group
                                   records straight to rank order: fused_kernels.hip.h), 0 pass by pass      */
    int big_buckets;            /* buckets of more than 3 072 entries (HB_CAP) the last build's hash grouping passed to
                                   k_bucket_big; 0 on paths that do not group buckets                       */
} ksp_stats;

const char* ksp_last_error(void);
int ksp_device_count(int* count);

/* ---- the hot path on device-resident data ------------------------------------------
 * Replaces the accumulate region of the reference, src/pairwise.cpp:194-237
 * (Combo::combinations + PAIRS_COUNTER::try_emplace_l), for sketches laid out as sorted
 * uint64 runs in HBM.  Source ids in the edges are dense indices 0..n_sources-1.      */
int ksp_engine_create(int device, ksp_engine** out);
void ksp_engine_destroy(ksp_engine* e);

/* Stage 1: merge the sorted runs of every block of 128 sources into one sorted
 * posting list per block (device).  d_keys: device pointer, concatenated sorted-unique
 * uint64 runs; d_weights: device pointer (one uint32 per key entry; the colour weight
 * w_c of src/pairwise.cpp:221) or NULL for weight 1; h_offsets: HOST pointer,
 * n_sources+1 element offsets; key_bits: significant bits of the largest key (at least the true width, at most 64),
 * 0 = find out on the device.  stream: hipStream_t (NULL = default stream).
 * Every argument is checked before the engine changes: a build refused with KSP_E_ARG or KSP_E_LIMIT leaves the last
 * build joinable and a pending join (ksp_engine_join_launch) collectable.  A build on another stream than a join still
 * pending on this engine is refused (KSP_E_ARG: nothing orders the two streams; collect the join first).  The same holds
 * for ksp_engine_build_slice, ksp_engine_build_postings[_slice], ksp_engine_slice_finish and ksp_engine_assemble.  */
int ksp_engine_build_blocks(ksp_engine* e, const uint64_t* d_keys, const uint32_t* d_weights,
                            const uint64_t* h_offsets, uint32_t n_sources, int key_bits, void* stream);

/* Tiles of the block-pair upper triangle in row-major order: tile t <-> (I, J), I <= J. */
uint64_t ksp_engine_num_tiles(const ksp_engine* e);
/* Source pairs covered by tiles [tile_begin, tile_end): the worst-case edge count.     */
uint64_t ksp_engine_tile_pairs(const ksp_engine* e, uint64_t tile_begin, uint64_t tile_end);
/* Tighter bound on the edges tiles [tile_begin, tile_end) can produce: the source pairs of the tiles
 * that share a key at all (stage 1 knows them; equals ksp_engine_tile_pairs in dense mode).       */
uint64_t ksp_engine_edge_bound(const ksp_engine* e, uint64_t tile_begin, uint64_t tile_end);
/* Tile ranges of equal estimated work for `nparts` GPUs: rank p joins tiles [cuts[p], cuts[p+1]).
 * cuts has nparts + 1 entries; every rank computes the same cuts from the same block lists.       */
int ksp_engine_balanced_cuts(const ksp_engine* e, uint32_t nparts, uint64_t* cuts);

/* Stage 2: join tiles [tile_begin, tile_end) and append every pair with shared > 0 to
 * d_edges (device buffer of `capacity` edges; order unspecified).  *h_count receives the
 * number of non-zero pairs; if it exceeds capacity the surplus was dropped and the call
 * returns KSP_E_OVERFLOW.  Synchronises `stream` before returning.                      */
int ksp_engine_join(ksp_engine* e, uint64_t tile_begin, uint64_t tile_end, ksp_edge* d_edges, uint64_t capacity,
                    uint64_t* h_count, void* stream);
/* The same in two halves, for callers that pipeline: _launch queues the join on `stream` and returns; _wait blocks
 * until it has finished and reports the count (one launched join per engine at a time: ksp_engine_join_launch,
 * ksp_engine_join and ksp_engine_join_to_host refuse with KSP_E_ARG while a launched join is not collected, and leave
 * it collectable).  Work queued on the same
 * stream after _launch — the next ksp_engine_build_blocks on this engine included — runs behind the join, so the
 * device does not idle while the host collects the count and hands the edges on (bench.py does exactly that). */
int ksp_engine_join_launch(ksp_engine* e, uint64_t tile_begin, uint64_t tile_end, ksp_edge* d_edges, uint64_t capacity, void* stream);
int ksp_engine_join_wait(ksp_engine* e, uint64_t* h_count);
/* A pipelined caller cannot retry an overflowed join: KSP_E_OVERFLOW is only reported by _wait, and by then the next
 * build has replaced the lists (and the tile numbering) the join ran on.  Size the buffer from ksp_engine_edge_bound
 * before _launch — the bound is exact enough to allocate by — and treat KSP_E_OVERFLOW from _wait as "this step's
 * result is incomplete, run the step again".                                                                     */

/* One step of a pipelined caller in one call: ksp_engine_build_blocks, the tile range of rank `part` of `nparts`
 * (ksp_engine_balanced_cuts; returned in range[0..1]), its edge bound (*bound) and ksp_engine_join_launch on that range
 * into d_edges — nothing between the build and the launch of its join but the cutting of the work list.
 * KSP_E_OVERFLOW: *bound + 1 > capacity, nothing was launched (grow the buffer, then ksp_engine_join_launch).
 * A join launched on this engine before the call (the previous step's) is collected on the way — it ran in front of
 * this build on the stream (a join pending on another stream makes the call fail with KSP_E_ARG, the join uncollected): *prev_count / *prev_status are what ksp_engine_join_wait would have returned for it,
 * *prev_ms_join (may be NULL) its kernel time.
 * Collect the join launched here with ksp_engine_join_wait, or with the next ksp_engine_step_launch.
 * A step launched this way puts NO timing events into the stream (an event record is a ~6 us bubble between two
 * kernels; a step had eleven): ksp_stats.ms_build / ms_sort / ms_join and *prev_ms_join of such a step read 0 unless
 * ksp_engine_set_profiling(e, 1) is on.  The host learns of the read-backs, of the work list's inputs and of the
 * join's count through sequence numbers in pinned memory that it polls.                                              */
int ksp_engine_step_launch(ksp_engine* e, const uint64_t* d_keys, const uint32_t* d_weights, const uint64_t* h_offsets,
                           uint32_t n_sources, int key_bits, uint32_t part, uint32_t nparts, ksp_edge* d_edges,
                           uint64_t capacity, uint64_t range[2], uint64_t* bound, uint64_t* prev_count, int* prev_status,
                           float* prev_ms_join, void* stream);

/* Join tiles [tile_begin, tile_end) and deliver the edges in HOST memory (h_edges: `capacity` edges, pinned memory
 * for full PCIe rate): the range is cut into pieces by the edge bound, piece k + 1 is joined while piece k is copied
 * on a stream of the engine's own.  For results of hundreds of MB (100k genomes: 45 M pairs), whose copy would
 * otherwise follow the join.  *h_count = pairs found; KSP_E_OVERFLOW if that exceeds capacity (*h_count is still the
 * full count: allocate and call again).  Returns when everything has arrived.  The pair map of the reference lives
 * in host memory throughout (src/pairwise.cpp:191); this is the step that gets the device's result there.          */
int ksp_engine_join_to_host(ksp_engine* e, uint64_t tile_begin, uint64_t tile_end, ksp_edge* h_edges, uint64_t capacity,
                            uint64_t* h_count, void* stream);

int ksp_engine_get_stats(const ksp_engine* e, ksp_stats* out);
/* How the last build made its block lists (diagnostics / tests): 0 no lists (nothing built, an empty build, assembled
 * slices), 1 the keyed split straight from the per-key group records, 2 the compacting chain (group records packed into
 * rank order first: KSP_MOVE=1, weighted or sparse inputs, more than 256 blocks), 3 the entries sorted by block,
 * 4 the bucket-resident stage 1 (KSP_FUSED=1).                                                                        */
int ksp_engine_lists_path(const ksp_engine* e, int* out);
/* Per-phase HIP-event times of stage 1 (the reference's own phase timers, src/pairwise.cpp:131-133,155,181,
 * 239, print wall-clock seconds per phase; this is their device-side counterpart).  set_profiling(1) makes
 * every later build record one event per phase start; phase_times returns the phases of the last build:
 * names[i] (static strings) and ms[i], at most cap of them; the return value is the count.               */
int ksp_engine_set_profiling(ksp_engine* e, int on);
int ksp_engine_phase_times(const ksp_engine* e, const char** names, float* ms, int cap);

/* Stage 1 from an inverted index instead of sketches: key k is held by the sources
 * d_sources[h_key_off[k] .. h_key_off[k+1]) (dense source indices, distinct inside a key, at least two per
 * key; keys in any order) and weighs d_key_weights[k] (NULL: 1).  This is exactly the reference's input —
 * `_color_to_sources.bin` + `_color_count.bin`, src/pairwise.cpp:128-170 — so the drop-in path hands its
 * colours over without transposing them into per-source runs and skips the engine's sort and prune.
 * The caller guarantees that every source's weights sum to less than 2^32.  Then ksp_engine_join as usual. */
int ksp_engine_build_postings(ksp_engine* e, const uint64_t* h_key_off, const uint32_t* d_sources,
                              const uint32_t* d_key_weights, uint32_t n_keys, uint32_t n_sources, void* stream);
/* One SLICE of such an index: any subset of its keys, every key with all its holders (same arguments, the offsets
 * starting at 0; fewer than 2^30 memberships per slice).  Stops at the source labels; from there the calls of a
 * key-range slice of sketches apply, plus the exchange of the counter bounds (ksp_engine_slice_labels, MIN over the
 * slices, ksp_engine_slice_bounds, SUM over the slices, ksp_engine_slice_set_bounds, ksp_engine_slice_finish, _sizes,
 * _export, ksp_engine_assemble).  The reference loads an index of any size (src/pairwise.cpp:95-111):
 * kspider_pairwise cuts one of 2^30 memberships or more into such slices by itself, and with $KSPIDER_DEVICES every
 * device builds the slice of 1 / n of the colours.                                                               */
int ksp_engine_build_postings_slice(ksp_engine* e, const uint64_t* h_key_off, const uint32_t* d_sources,
                                    const uint32_t* d_key_weights, uint32_t n_keys, uint32_t n_sources, void* stream);

/* ---- stage 1 sharded over GPUs (one process per GPU) ---------------------------------------
 * Every rank holds the full sketch set; rank `part` of `nparts` sorts and prunes the keys of its
 * 1/nparts share of the hash range only (ksp_engine_build_slice).  The engine orders the sources by a
 * label derived from the shared keys, so the ranks first combine their labels (ksp_engine_slice_labels,
 * element-wise MIN all-reduce of n_sources uint32 over RCCL, ksp_engine_slice_finish) and then build
 * their slices of the block lists in that common order.  The slices are exchanged by the caller
 * (all-gather: kspider_amd/dist.py) and every rank turns the gathered slices into the full block lists
 * (ksp_engine_assemble) before ksp_engine_join.
 *   slice_labels: copies the slice's n_sources labels into a device buffer.
 *   slice_finish: d_labels = the combined labels (device; NULL keeps the slice's own: single slice
 *                tests only — every rank must use the same labels).
 *   slice_sizes: out[0] padded list length L (uint32 entries of d_brk / d_info / d_bw),
 *                out[1] distinct keys, out[2] 128-bit posting masks, out[3] block keys.
 *   slice_export: copies the slice into caller buffers (device pointers): d_brk/d_info[/d_bw] L
 *                entries, d_blk_raw/d_blk_pos n_blocks+1 entries, d_big out[2] x 16 bytes.
 *   assemble:    h_sizes = nparts x 4 values as reported by slice_sizes (host); the *_all buffers
 *                hold the parts back to back with strides lstride (entries) / n_blocks+1 /
 *                bigstride (16-byte masks); must run on an engine that built one of the slices. */
int ksp_engine_build_slice(ksp_engine* e, const uint64_t* d_keys, const uint32_t* d_weights,
                           const uint64_t* h_offsets, uint32_t n_sources, int key_bits, uint32_t part,
                           uint32_t nparts, void* stream);
int ksp_engine_slice_labels(ksp_engine* e, uint32_t* d_labels, void* stream);
int ksp_engine_slice_finish(ksp_engine* e, const uint32_t* d_labels, void* stream);
/* The bound of every source's pair counters as the slice knows it (n_sources uint32: number of keys / weight sum), and
 * the combined bounds handed back before ksp_engine_slice_finish.  Slices of sketches report full bounds (every slice
 * sees every source's whole run): the exchange is not needed.  Slices of an inverted index (ksp_engine_build_postings_slice)
 * see their own keys only: the caller adds the slices' bounds up element by element (a SUM all-reduce) and sets the
 * sums on every slice.  A slice of an index finished without them takes every source for one that needs 32-bit
 * counters (correct, slower): one slice's share says nothing about the sums the assembled lists reach.        */
int ksp_engine_slice_bounds(ksp_engine* e, uint32_t* d_bounds, void* stream);
int ksp_engine_slice_set_bounds(ksp_engine* e, const uint32_t* d_bounds, void* stream);
int ksp_engine_slice_sizes(const ksp_engine* e, uint64_t out[4]);
int ksp_engine_slice_export(ksp_engine* e, uint32_t* d_brk, uint32_t* d_info, uint32_t* d_bw, uint32_t* d_blk_raw,
                            uint32_t* d_blk_pos, void* d_big, void* stream);
int ksp_engine_assemble(ksp_engine* e, uint32_t nparts, const uint64_t* h_sizes, const uint32_t* d_brk_all,
                        const uint32_t* d_info_all, const uint32_t* d_bw_all, uint64_t lstride,
                        const uint32_t* d_blk_raw_all, const uint32_t* d_blk_pos_all, const void* d_big_all,
                        uint64_t bigstride, void* stream);

/* ---- thin device-memory helpers so that FFI callers need no HIP binding ------------- */
int ksp_device_malloc(int device, uint64_t bytes, void** d_ptr);
int ksp_device_free(void* d_ptr);
int ksp_memcpy_h2d(void* d_dst, const void* h_src, uint64_t bytes);
int ksp_memcpy_d2h(void* h_dst, const void* d_src, uint64_t bytes);

/* ---- host-buffer convenience (H2D + both stages + D2H), edges sorted by (s1, s2) ---- */
int ksp_pairwise_host(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                      int device, ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats);
/* Same for an inverted index in host memory (see ksp_engine_build_postings). */
int ksp_pairwise_postings_host(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights,
                               uint32_t n_keys, uint32_t n_sources, int device, ksp_edge** out_edges,
                               uint64_t* n_edges, ksp_stats* stats);
void ksp_free(void* p);
/* The same two jobs on several GPUs of one node, one host thread and one engine per device (devices[] may name a
 * device twice: two engines share it — used by the single-GPU tests).  This is what $KSPIDER_DEVICES selects
 * behind kspider_pairwise() / kSpider::pairwise() (north star: the N x N pair space sharded over the GPUs of a
 * node): sketch input is built in hash-range slices, one per device, exchanged device to device; an inverted
 * index is built on every device; every device joins a tile range of equal estimated work; the edges are
 * gathered to devices[0] (peer copies over xGMI), sorted there and returned in pinned host memory.        */
int ksp_pairwise_host_multi(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                            const int* devices, int n_devices, ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats);
int ksp_pairwise_postings_host_multi(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights,
                                     uint32_t n_keys, uint32_t n_sources, const int* devices, int n_devices,
                                     ksp_edge** out_edges, uint64_t* n_edges, ksp_stats* stats);

/* ---- the reference entry point ------------------------------------------------------
 * Same contract as kSpider::pairwise(string index_prefix, int user_threads)
 * (include/kSpider.hpp:11): reads PREFIX_color_to_sources.bin, PREFIX_color_count.bin,
 * PREFIX_groupID_to_kmerCount.bin, writes PREFIX_kSpider_seqToKmersNo.tsv and
 * PREFIX_kSpider_pairwise.tsv.  Device = $KSPIDER_DEVICE (default 0); $KSPIDER_DEVICES=0,1,...
 * shards the job over several GPUs (ksp_pairwise_postings_host_multi) — same output files.      */
int kspider_pairwise(const char* index_prefix, int user_threads);

/* ---- direct sketch inputs ----------------------------------
 * kspider_pairwise_sigs: sourmash signatures (every .sig file of DIR) -> pairwise TSVs in one go; what
 *   kSpider::sourmash_sigs_indexing(sigs_dir, kSize) (include/kSpider.hpp:18,
 *   src/sourmash_indexing.cpp:52) followed by kSpider::pairwise() computes, with the same group-ID
 *   assignment (glob order), first signature with ksize == kSize, PREFIX.namesMap format.
 * kspider_pairwise_bins: sketches stored as phmap::flat_hash_set<uint64_t> dumps, every .bin file of DIR (the
 *   input format of kSpider::bins_indexing, src/bins_indexing.cpp:98-182).
 * out_prefix NULL/"" -> basename(DIR) in the current directory, as the reference does.
 * Writes PREFIX.namesMap, PREFIX_kSpider_seqToKmersNo.tsv, PREFIX_kSpider_pairwise.tsv.        */
int kspider_pairwise_sigs(const char* sigs_dir, int kSize, const char* out_prefix, int user_threads);
int kspider_pairwise_bins(const char* bins_dir, const char* out_prefix, int user_threads);

/* ---- clustering -------------------------------------------------------
 * kspider_cluster: what `kSpider cluster -i PREFIX -d DIST -c CUTOFF` does (pykSpider/kSpider2/
 *   ks_clustering.py:63-137, 150-163): reads PREFIX.namesMap, PREFIX_kSpider_seqToKmersNo.tsv and
 *   PREFIX_kSpider_pairwise.tsv (dist_type "ani": also PREFIX_kSpider_pairwise.ani_col.tsv), keeps the rows
 *   whose column dist_type ("min_cont" 3, "avg_cont" 4, "max_cont" 5; NULL = "max_cont") times 100 is not
 *   below cutoff * 100 (cutoff in [0, 1]), finds the connected components ON THE GPU and writes one line of
 *   comma-separated names per component to PREFIX_kSpider_clusters_<cutoff*100>%.tsv.  Components are
 *   written in order of their smallest node, names in node order (the reference: rustworkx set order).
 * ksp_components: the device part alone — connected components of an undirected edge list (host arrays
 *   of node indices < n_nodes); h_label[v] = smallest node index of v's component.                      */
int kspider_cluster(const char* index_prefix, const char* dist_type, double cutoff);
int ksp_components(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, uint64_t n_edges,
                   uint32_t* h_label);
/* Clustering from HBM — what SURVEY 8f N4 is for: the pairs never leave the device as text.
 * ksp_components_edges: components straight over the join's edge records.  d_edges: `n_edges` ksp_edge records in
 *   DEVICE memory (as ksp_engine_join leaves them; node = source index), d_kmer_counts[v] = k-mer count of source v
 *   (device memory).  An edge counts when its containment column dist_col (3 min, 4 avg, 5 max; single-precision maths
 *   of src/pairwise.cpp:260-264) passes the reference's test: text of the float with 6 significant digits -> float ->
 *   x 100 -> not below cutoff x 100 (ks_clustering.py:101-105; a NaN passes).  That test is monotone in the float, so
 *   the device compares against the one critical float found on the host — the same rows pass, digit for digit.
 *   h_label[v] = smallest source index of v's component.
 * kspider_pairwise_and_cluster: `kSpider pairwise` followed by `kSpider cluster` (ks_clustering.py:63-137) in ONE
 *   device pass: writes PREFIX_kSpider_seqToKmersNo.tsv and PREFIX_kSpider_pairwise.tsv exactly as kspider_pairwise
 *   and PREFIX_kSpider_clusters_<cutoff*100>%.tsv exactly as kspider_cluster would from that TSV — but the components
 *   come from the edges while they are in HBM (the TSV is never read back).  dist_type: "min_cont", "avg_cont",
 *   "max_cont" (NULL / ""); "ani" is refused here: kspider_pairwise_ani_and_cluster is the ANI form.  Reads
 *   PREFIX.namesMap like kspider_cluster.                                                                          */
int ksp_components_edges(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                         int dist_col, double cutoff, uint32_t* h_label);
int kspider_pairwise_and_cluster(const char* index_prefix, int user_threads, const char* dist_type, double cutoff);

/* ---- ANI (`kSpider pairwise --estimate-ani`, then `kSpider cluster -d ani`) -------------------------
 * The value of a pairwise row is what pykSpider/kSpider2/ks_pairwise.py:64-82 writes: columns 3 and 5 (min / max
 * containment) read as Python floats from their 6-significant-digit text, each turned into sourmash's point-estimate ANI
 *   g(c) = 0.0 if c <= 0.0001;  1.0 if c >= 0.9999;  1 - (1.0 - c ** (1.0 / k)) otherwise
 * and the row's value (g(min) + g(max)) / 2.0, written with Python's repr.  k is the first line of PREFIX.extra
 * (:44-46).  sourmash's scale and the k-mer counts only feed a quantity .ani discards: the scale must still be > 0 (:41)
 * and every id of a row must be in PREFIX_kSpider_seqToKmersNo.tsv (:77-78).  A NaN containment has no ANI: an error.
 * The formula is restated from sourmash, which is not vendored: no reference-generated output pins it.
 * kspider_estimate_ani: `kSpider pairwise -i PREFIX --estimate-ani -s SCALE` (ks_pairwise.py:29-84) over existing files:
 *   reads PREFIX.extra, PREFIX_kSpider_seqToKmersNo.tsv and PREFIX_kSpider_pairwise.tsv (any producer, rows in any order)
 *   and writes PREFIX_kSpider_pairwise.ani_col.tsv ("avg_ani", then one line per row in the TSV's order) through a
 *   .partial file; on any error nothing is written.  Host only, user_threads threads parse and format.
 * kspider_pairwise_ani: kspider_pairwise followed by kspider_estimate_ani in one pass: the same two TSVs byte for byte,
 *   plus the ANI column, evaluated from the rows' floats (no text is read back).
 * kspider_pairwise_ani_and_cluster: also `kSpider cluster -d ani -c CUTOFF` (ks_clustering.py:63-137): the components
 *   come from the edges while they are in HBM (the device evaluates the ANI of every edge, an edge counts when
 *   ani * 100 is not below cutoff * 100) and go to PREFIX_kSpider_clusters_<cutoff*100>%.tsv as kspider_cluster
 *   writes it.  Every kept edge counts (the reference's batch loses one edge per 10 000 001: INTEGRATION.md).
 * ksp_edges_ani: d_ani[e] = the ANI of edge record e (all pointers DEVICE memory, as ksp_components_edges takes them);
 *   KSP_E_ARG if any edge has a NaN containment (its d_ani is NaN).
 * ksp_components_edges_ani: ksp_components_edges with the ANI column (ksize) as the distance.                      */
int kspider_estimate_ani(const char* index_prefix, int user_threads, int64_t scale);
int kspider_pairwise_ani(const char* index_prefix, int user_threads, int64_t scale);
int kspider_pairwise_ani_and_cluster(const char* index_prefix, int user_threads, int64_t scale, double cutoff);
int ksp_edges_ani(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int ksize, double* d_ani);
int ksp_components_edges_ani(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                             int ksize, double cutoff, uint32_t* h_label);

/* ---- export (`kSpider export`) ----------------------------------------------------------------------
 * kspider_export: what `kSpider export -i PREFIX -d DIST [--newick] [-o OUT]` writes (pykSpider/kSpider2/ks_export.py):
 *   reads PREFIX.namesMap, PREFIX_kSpider_seqToKmersNo.tsv (must parse; values unused) and PREFIX_kSpider_pairwise.tsv
 *   (dist_type "ani": also PREFIX_kSpider_pairwise.ani_col.tsv, line for line), dist_type "min_cont" 3, "avg_cont" 4,
 *   "max_cont" 5 (NULL / "") or "ani", and writes
 *     OUT_pairwise.tsv   "grp1\tgrp2\t<dist>" ("source1\tsource2\tani"), then both names and repr() of the value per row;
 *     OUT_distmat.tsv    pandas' to_csv(sep='\t') of the N x N matrix over the names that occur (sorted): cell (a, b) =
 *                        (b, a) = 1 - value, the fill 0 printed "0.0" in a column with a non-NaN value and "0" in a column
 *                        whose values are all NaN (pandas' int64 downcast); a NaN value is the fill;
 *     OUT.newick         (newick != 0) scipy's linkage(M, 'single') of that matrix as read_csv reads it back (Euclidean
 *                        distances between ROWS) ON THE GPU, printed as the reference's get_newick prints to_tree.
 *   out_prefix NULL / "": kSpider_<basename(PREFIX)>_pairwise.tsv, ..._distmat.tsv, kSpider_<basename>.newick in the
 *   current directory.  Every file goes through OUT....partial and a rename; on any error none is left behind.
 *   Refused up front (before any file is written, unlike the reference, which writes two files and then raises):
 *   KSP_E_ARG for an unknown distance, a row id missing from .namesMap (ids are matched by their text, as the reference's
 *   dict does: '01' is not '1'), a repeated unordered pair or a self pair, and with newick fewer than 2 nodes, a
 *   non-finite 1 - value or a non-finite distance between two rows (scipy refuses it; found on the device, still
 *   before any file is written); KSP_E_LIMIT with newick above 65 536 nodes or when the two
 *   N x N double matrices do not fit the device's free memory.  Device = $KSPIDER_DEVICE (default 0).
 * ksp_single_linkage_rows: the device part alone.  d_rows: an n x n row-major double matrix in DEVICE memory (not
 *   changed); h_Z receives (n - 1) x 4 doubles equal to scipy.cluster.hierarchy.linkage(rows, 'single') bit for bit for
 *   any finite matrix.  KSP_E_ARG when a distance between two rows is not finite (a cell of 1e200 squares to inf), as
 *   scipy refuses it.  KSP_E_LIMIT above n = 65 536 (checked first) or when the n x n distance matrix does not fit.
 * ksp_single_linkage_prim: the same computation, but h_prim receives Prim's (n - 1) x 4 rows (x, y, height, m) in the
 *   order scipy's mst_single_linkage finds them, before the sort and the relabel: x is the node merged last (scipy's
 *   Z[k, 0]), m the merged node whose row set D[y], so that height = distance(m, y) exactly (tests check every edge).
 * ksp_row_distances: a test entry — h_dist (host memory) receives the n x n row-major matrix of distances between the
 *   rows of d_rows that both entries above compute on the device and Prim reads (scipy's pdist(rows) in square form, bit
 *   for bit), launched by the same code.  The checks and their order are theirs: KSP_E_LIMIT above n = 65 536 (before
 *   any device call), KSP_E_ARG for n < 2 or a NULL pointer, KSP_E_LIMIT when the matrix does not fit the device's free
 *   memory, KSP_E_ARG when a distance is not finite.
 * ksp_csv_float: host only — the text of one cell as pandas' read_csv parses it (precise_xstrtod, not correctly
 *   rounded; "inf", "-inf", "nan" too).  KSP_E_ARG when the text is not a number.                                     */
int kspider_export(const char* index_prefix, const char* dist_type, int newick, const char* out_prefix);
int ksp_single_linkage_rows(int device, uint32_t n, const double* d_rows, double* h_Z);
int ksp_single_linkage_prim(int device, uint32_t n, const double* d_rows, double* h_prim);
int ksp_row_distances(int device, uint32_t n, const double* d_rows, double* h_dist);
int ksp_csv_float(const char* text, double* out);

/* ---- representative sketches (the reference's tool `repr_sketches`, apps/repr_sketches.cpp:27-33,38-43) -----------------
 * The tool reads PREFIX_kSpider_pairwise.tsv: a row passes when stof(text of column 4, avg_containment) > 0.20 (the float
 * promoted to double, strictly; a NaN never passes), a passing row counts one neighbour for both of its ids, and the ids
 * with a count are printed as "id: count" lines, largest count first.  The order among equal counts is not pinned by the
 * reference (an unstable sort over a hash map's iteration order); here it is canonical: count descending, then id
 * ascending.  The text of a float has 6 significant digits, so the test on a float is not `v > threshold`: it is
 * monotone, and one critical float decides it (0.20: bit pattern 0x3e4cccac, 0.199999511 — it prints "0.2").
 * ksp_edges_degrees: the neighbour counts straight over the join's edge records.  d_edges: `n_edges` ksp_edge records in
 *   DEVICE memory, in any order, every record counted; d_kmer_counts[v] = k-mer count of source v (device memory); dist_col
 *   3 min, 4 avg (the reference's), 5 max containment, single-precision maths of src/pairwise.cpp:260-264.  h_degree[v] (host,
 *   n_nodes entries) = number of records naming v whose column passes the text test against `threshold`.  An edge naming a
 *   node >= n_nodes is the caller's error, as for ksp_components_edges: it is not counted and not reported.
 * ksp_edges_repr: the same counts ranked on the device: h_node[i] / h_count[i] for i < *n_ranked are the nodes with a
 *   non-zero count in (count descending, node ascending) order; both arrays hold n_nodes entries.
 *   Both: KSP_E_ARG for a NULL pointer with n_edges > 0, a column other than 3 / 4 / 5 and a NaN threshold; KSP_E_LIMIT for
 *   2^32 edges or more (the counters are 32-bit).  n_edges = 0: all-zero degrees, *n_ranked = 0, no kernel runs.
 * ksp_repr_critical: host only — the smallest non-negative float that passes the text test for `threshold`
 *   ("%.6g" text -> strtof -> as double -> > threshold); *none_pass = 1 when not even +inf passes (nothing is counted).
 * kspider_repr_sketches: the tool itself over an existing TSV of any producer, rows in any order: the host parses columns
 *   0, 1 and dist_type ("min_cont" 3, "avg_cont" 4 = NULL / "", "max_cont" 5; "ani" is refused with KSP_E_ARG) and applies
 *   the text test, the device counts and ranks.  The reference call is (tsv, "avg_cont", 0.20, NULL).  out_path NULL / "":
 *   stdout, as the reference; otherwise through out_path.partial and a rename, and on any error nothing is left behind.
 *   KSP_E_IO (naming the line) for a row with too few columns or a value that is not a number / an id that is not a decimal
 *   integer (the reference throws there); KSP_E_ARG for an id outside [0, 2^31 - 1] (the reference reads ids with stoi).
 *   Device = $KSPIDER_DEVICE (default 0).
 * kspider_pairwise_and_repr: kspider_pairwise followed by the tool in ONE device pass: the same two TSVs byte for byte, plus
 *   the ranking (out_path NULL / "": PREFIX_kSpider_repr_sketches.txt), counted from the edges while they are in HBM; ids
 *   are the index's group ids.  KSP_E_LIMIT, before any file is written, when a group id exceeds 2^31 - 1.  Works with
 *   $KSPIDER_DEVICES like kspider_pairwise.                                                                              */
int ksp_edges_degrees(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                      int dist_col, double threshold, uint32_t* h_degree);
int ksp_edges_repr(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                   int dist_col, double threshold, uint32_t* h_node, uint32_t* h_count, uint32_t* n_ranked);
int ksp_repr_critical(double threshold, float* vcrit, int* none_pass);
int kspider_repr_sketches(const char* pairwise_tsv, const char* dist_type, double threshold, const char* out_path);
int kspider_pairwise_and_repr(const char* index_prefix, int user_threads, const char* dist_type, double threshold,
                              const char* out_path);

/* ---- the containment cut: a minimum containment on the producer -------------------------------------------
 * A row is kept exactly when `kSpider cluster -d DIST -c CUTOFF` would keep it (ks_clustering.py:101-105): text of the
 * column's float with 6 significant digits -> Python float -> x 100 -> not below cutoff x 100; a NaN row is kept.  The test
 * is monotone in the float, so the device makes one compare against the critical float, as ksp_components_edges does.
 * Guarantee: after kspider_pairwise_cut(PREFIX, T, D, c), kspider_cluster(PREFIX, D, c') for any c' with
 * c' x 100 >= c x 100 writes the same cluster file, byte for byte, as over the full TSV.
 * ksp_edges_cut: the device part alone — a STABLE compaction.  d_edges: `n_edges` ksp_edge records in DEVICE memory, in any
 *   order, never written; d_kmer_counts[v] = k-mer count of source v (device memory); dist_col 3 min, 4 avg, 5 max
 *   containment, single-precision maths of src/pairwise.cpp:260-264.  The kept records go to d_out[0 .. *n_kept) (device
 *   memory with room for n_edges records, or for as many as are kept) in their input order; d_out[*n_kept ..] is not written.
 *   KSP_E_ARG for a NULL pointer with n_edges > 0, a column other than 3 / 4 / 5, a NaN cut-off and d_out overlapping
 *   d_edges.  n_edges = 0: *n_kept = 0, no kernel runs.  Every count and offset is 64-bit: 2^32 records or more are not
 *   refused.  An edge naming a node outside the counts is the caller's error, as for ksp_components_edges.
 *   KSP_CUT_CHUNK_EDGES: records per chunk of the two passes (one 64-bit count per chunk).
 * ksp_pairwise_host_cut: ksp_pairwise_host_multi with the cut made on every device directly after its join: only the kept
 *   edges are gathered, sorted and copied.  kmer_counts[v] = k-mer count of source v (host; NULL: the run lengths
 *   offsets[v + 1] - offsets[v]).  *out_edges / *n_edges: the kept edges sorted by (source_1, source_2) (ksp_free);
 *   *n_found (may be NULL): the edges before the cut; stats->last_edges is the kept total.  KSP_E_ARG as above.
 * kspider_pairwise_cut: kspider_pairwise with the cut: PREFIX_kSpider_pairwise.tsv holds the kept rows in (source_1, source_2)
 *   order, rows that exist only with shared_kmers = 0 (colours of weight 0) tested the same way on the host;
 *   PREFIX_kSpider_seqToKmersNo.tsv is never affected.  dist_type "min_cont", "avg_cont", "max_cont" (NULL / "": max_cont);
 *   "ani" and a cut-off outside kspider_cluster's range [0, 1] (or NaN) are refused with KSP_E_ARG before any file is
 *   written.  Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES like kspider_pairwise; with $KSPIDER_VERBOSE one line reports
 *   the rows found and kept.  The cut TSV is a valid input of kspider_cluster / kspider_export / kspider_repr_sketches at
 *   cut-offs not below the cut.                                                                                          */
#define KSP_CUT_CHUNK_EDGES 2048u
int ksp_edges_cut(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, double cutoff,
                  ksp_edge* d_out, uint64_t* n_kept);
int ksp_pairwise_host_cut(const uint64_t* keys, const uint32_t* weights, const uint64_t* offsets, uint32_t n_sources,
                          const uint32_t* kmer_counts, int dist_col, double cutoff, const int* devices, int n_devices,
                          ksp_edge** out_edges, uint64_t* n_edges, uint64_t* n_found, ksp_stats* stats);
int kspider_pairwise_cut(const char* index_prefix, int user_threads, const char* dist_type, double cutoff);

/* ---- the cut-off ladder: the clusters at a list of cut-offs in one device pass ----------------------------
 * "Kept" means for every cut-off what it means to kspider_cluster / ksp_components_edges: columns 3 / 4 / 5 against the
 * critical float of the cut-off (a NaN is kept), the ANI column (file path only) by !(value x 100 < cutoff x 100) in double.
 * Ordered by strictness the cut-offs an edge passes are the L least strict ones; L, 0 .. n_cutoffs, is the edge's level (a
 * NaN: n_cutoffs), and the clustering of the cut-off at strictness rank r is the components of the edges with L > r.  The
 * device classifies every edge once, sorts the edges of level >= 1 into one band per level and computes the components
 * band by band, strictest first, continuing on the labels of the ranks before.  Cut-offs come in any order and may repeat;
 * results are in the caller's order.  1 <= n_cutoffs <= KSP_SWEEP_MAX_CUTOFFS (a level fits a byte), else KSP_E_ARG.
 * ksp_components_edges_sweep: d_edges: `n_edges` ksp_edge records in DEVICE memory, never written; d_kmer_counts and dist_col
 *   (3 / 4 / 5) as for ksp_components_edges.  h_labels: n_cutoffs x n_nodes, row i = the labels ksp_components_edges gives for
 *   cutoffs[i] (label = smallest node of the component); h_kept (may be NULL): edges kept per cut-off.  KSP_E_ARG for a NULL
 *   pointer, a column other than 3 / 4 / 5 and a NaN cut-off; KSP_E_LIMIT, before anything is written, when the level bytes
 *   (n_edges), the bands (8 bytes per edge of level >= 1) and (n_cutoffs + 1) x n_nodes labels do not fit the device's free
 *   memory.  $KSP_SWEEP_MAX_WORKGROUPS caps the grids of both passes (tests).  KSP_SWEEP_CHUNK_EDGES: records per chunk.
 * ksp_components_sweep: the same for HOST edges that are already classified: level[e] in 0 .. n_levels; row r of h_labels
 *   (n_levels x n_nodes) = the components of the edges with level > r.  KSP_E_ARG for a level above n_levels and for an edge
 *   of level >= 1 naming a node >= n_nodes (an edge of level 0 is never looked at).
 * kspider_cluster_sweep: kspider_cluster at every cut-off of the list from ONE reading of its files (same validation, same
 *   refusals, "ani" through PREFIX_kSpider_pairwise.ani_col.tsv): one PREFIX_kSpider_clusters_<cutoff*100>%.tsv per distinct
 *   cut-off, name and bytes as kspider_cluster writes them (a repeated name is written once), and
 *   PREFIX_kSpider_cluster_sweep_<dist_type>.tsv: "cutoff_percent\tedges\tclusters\tsingletons\tlargest", one row per distinct
 *   cut-off, ascending; cutoff_percent is the text in the cluster file's name, edges the rows kept.  Every refusal comes
 *   before any file is written; on an error no new file and no .partial is left.
 * kspider_pairwise_and_cluster_sweep: kspider_pairwise_and_cluster with the list: the pairwise TSV of kspider_pairwise, the
 *   ladder from the gathered, sorted edges on the first device, rows that exist only with shared_kmers = 0 classified on the
 *   host and united into every rank they pass; the same cluster files and summary.  "ani" is refused, as there.        */
#define KSP_SWEEP_CHUNK_EDGES 2048u
#define KSP_SWEEP_MAX_CUTOFFS 255u
int ksp_components_edges_sweep(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                               int dist_col, const double* cutoffs, uint32_t n_cutoffs, uint32_t* h_labels, uint64_t* h_kept);
int ksp_components_sweep(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint8_t* h_level, uint64_t n_edges,
                         uint32_t n_levels, uint32_t* h_labels);
int kspider_cluster_sweep(const char* index_prefix, const char* dist_type, const double* cutoffs, uint32_t n_cutoffs);
int kspider_pairwise_and_cluster_sweep(const char* index_prefix, int user_threads, const char* dist_type, const double* cutoffs,
                                       uint32_t n_cutoffs);

/* ---- the single-linkage tree of the containment graph: a maximum spanning forest on the device ---------------
 * The clusters of kspider_cluster at EVERY cut-off are the single-linkage hierarchy of the graph whose edges are the pairwise
 * rows, and a maximum spanning forest of that graph fixes it: at most N - 1 rows, whose components at any cut-off are the
 * components of all rows at that cut-off.  Order of edges, a strict total order: the column value, larger first, a NaN above
 * every number (a NaN row is kept at every cut-off), ties by record index, lower first; so the forest is unique.  Every record
 * is an edge, whatever its `shared`, except a record with source_1 == source_2, which is skipped; a pair may repeat.
 * Guarantee: kspider_cluster_from_tree at any cut-off in [0, 1] writes the cluster file kspider_cluster writes over the full
 * TSV, byte for byte (tests/test_tree_gpu.py::test_tree_files).
 * ksp_edges_forest: d_edges: `n_edges` ksp_edge records in DEVICE memory, never written; d_kmer_counts and dist_col (3 / 4 / 5)
 *   as for ksp_components_edges, the value compared as the float the pairwise writer computes.  h_index (host, room for
 *   min(n_nodes - 1, n_edges) entries) receives the indices of the forest's records in merge order — NaN first, then value
 *   descending, then lower index — and *n_forest their number; nothing behind them is written.  KSP_E_ARG for a NULL pointer
 *   with n_edges > 0, a NULL n_forest and a column other than 3 / 4 / 5; KSP_E_LIMIT for 2^32 - 1 records or more (the index is
 *   half of the 64-bit key), and, before anything is written to the caller, when 12 bytes per record plus 16 bytes per node do
 *   not fit the device's free memory; KSP_E_HIP with a message, never a spin, should a round not flatten in 34 jump passes or
 *   the rounds exceed ceil(log2(n_nodes)) + 2.  n_edges = 0: *n_forest = 0, no kernel runs.  An endpoint >= n_nodes is the
 *   caller's error, as for ksp_components_edges.  $KSP_TREE_MAX_WORKGROUPS caps the grids of the edge passes (tests).
 *   KSP_TREE_CHUNK_EDGES: records per chunk.
 * ksp_forest_ranked: the same forest for HOST edges whose weights the caller has ranked: a higher h_rank merges earlier, ties
 *   go to the lower index.  KSP_E_ARG for an endpoint >= n_nodes; the other refusals as above.
 * kspider_tree: reads what kspider_cluster reads, with the same validation and the same refusals (every row is an edge here, so
 *   every row's ids must be rows of .namesMap), each before any file is written; "ani" goes through
 *   PREFIX_kSpider_pairwise.ani_col.tsv.  The weight of a row is the value kspider_cluster tests, float(text) x 100, a NaN the
 *   top; the host sorts the distinct weights into ranks, the device finds the forest.  Writes PREFIX_kSpider_tree_<dist_type>.tsv:
 *   "source_1\tsource_2\t<dist_type>\tmerged_size", one row per forest edge with the row's two ids, the text of its value exactly
 *   as it stands in the input and the size of the cluster that merge creates; rows by value descending (NaN first), then
 *   (source_1, source_2).  newick != 0: also PREFIX_kSpider_tree_<dist_type>.newick, names from .namesMap, the height of a merge
 *   1 - value clamped to [0, 1] (NaN: 0), a branch length parent height minus child height printed "%.6g", the child holding
 *   source_1 first; clusters that never join go, in order of their smallest node, under one root at height 1 (no shared
 *   k-mers); a single node is "name;".  Every file goes through .partial and a rename; on an error nothing new is left behind.
 *   Device = $KSPIDER_DEVICE (default 0).
 * kspider_pairwise_and_tree: kspider_pairwise's two TSVs, byte for byte, plus the same tree files, the forest taken from the
 *   gathered, sorted edges on the first device; rows that exist only with shared_kmers = 0 (colours of weight 0) are united in
 *   on the host after the device's forest, in (source_1, source_2) order.  "ani" is refused with KSP_E_ARG, as in the sibling
 *   calls.  Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES.  This path orders the rows by their FLOAT, which is finer than the
 *   6-digit text kspider_tree reads, so among rows of equal text the two may choose different ones: both files are maximum
 *   spanning forests for the text values and their cuts are equal, but the files are not promised to be byte-equal.
 * kspider_cluster_from_tree: host only.  Reads .namesMap and PREFIX_kSpider_tree_<dist_type>.tsv, keeps the rows kspider_cluster
 *   would keep (the same test on the same text; for "ani" its double test), unites them and writes
 *   PREFIX_kSpider_clusters_<cutoff*100>%.tsv as kspider_cluster does.  KSP_E_IO for a missing or malformed file and for a row
 *   whose id is not a row of .namesMap; KSP_E_ARG for an unknown distance.                                                  */
#define KSP_TREE_CHUNK_EDGES 2048u
int ksp_edges_forest(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                     int dist_col, uint32_t* h_index, uint32_t* n_forest);
int ksp_forest_ranked(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_rank,
                      uint64_t n_edges, uint32_t* h_index, uint32_t* n_forest);
int kspider_tree(const char* index_prefix, const char* dist_type, int newick);
int kspider_pairwise_and_tree(const char* index_prefix, int user_threads, const char* dist_type, int newick);
int kspider_cluster_from_tree(const char* index_prefix, const char* dist_type, double cutoff);

/* ---- dereplication: greedy representatives and their members, from the edges in HBM -------------------------
 * What a user of the `repr_sketches` ranking goes on to compute: which sources to keep and, for every other source, which
 * kept source stands for it.  A record is KEPT when its column passes the text test of `repr_sketches` ("%.6g" text -> strtof
 * -> as double -> > threshold; on the device one compare against the critical float of ksp_repr_critical; a NaN never passes).
 * degree[v] is what ksp_edges_degrees returns (a repeated pair counts again, a self pair adds 2).  All n_nodes nodes are
 * ranked by (degree descending, node ascending): ksp_edges_repr's order, then the nodes of degree 0 in node order.  Walking
 * the nodes in rank order, a node becomes a REPRESENTATIVE unless one of its kept neighbours of smaller rank is one; otherwise
 * it becomes a MEMBER of the smallest-ranked representative among its kept neighbours (cd-hit's rule: the first
 * representative that covers it, whatever the value), through the lowest-index kept record between the two.  Self pairs take
 * no part in the selection.  So no two representatives share a kept record, every member shares one with its representative,
 * every node of degree 0 is a representative, and only `via` depends on the order of the records.
 * ksp_edges_dereplicate: d_edges: `n_edges` ksp_edge records in DEVICE memory, in any order, never written; d_kmer_counts and
 *   dist_col (3 / 4 / 5) as for ksp_edges_degrees.  Host arrays of n_nodes entries: h_rep[v] = the representative of v (v
 *   itself: v is one), h_via[v] = the index of the assigning record (0xFFFFFFFF for a representative), h_rank[v] = the position
 *   of v in the order above, h_degree[v]; h_via, h_rank and h_degree may be NULL.  *n_reps = the representatives.  A record
 *   naming a node >= n_nodes is the caller's error and is ignored.  KSP_E_ARG for a NULL pointer with n_edges > 0, a NULL
 *   n_reps, a column other than 3 / 4 / 5 and a NaN threshold; KSP_E_LIMIT for 2^32 - 1 records or more (the index is half of
 *   a 64-bit key and 0xFFFFFFFF is "none") and, before anything is written to the caller, when 52 bytes per node, 16 per 2 048
 *   records and 20 per kept pair do not fit the device's free memory; KSP_E_HIP with a message, never a spin, should the
 *   rounds exceed n_nodes + 1.  n_edges = 0, or a threshold not even +inf passes: every node is its own representative,
 *   *n_reps = n_nodes, ranks in node order, no kernel runs.  $KSP_DEREP_MAX_WORKGROUPS caps the grids of the edge passes
 *   (tests), $KSP_DEREP_TAIL=0 keeps the host-driven rounds to the end (same results).  KSP_DEREP_CHUNK_EDGES: entries per
 *   chunk of the edge passes.  KSP_DEREP_TAIL_PAIRS: at that many live pairs or fewer one workgroup finishes the rounds
 *   (UNMEASURED: DESIGN.md 7h).
 * kspider_dereplicate: reads what kspider_cluster reads, with the same validation and the same refusals, each before any file
 *   is written; the ids of a passing row must be rows of .namesMap.  The host applies the text test to the text as it stands,
 *   the device makes the selection over the passing rows.  dist_type "min_cont", "avg_cont" (NULL / ""), "max_cont"; "ani", a
 *   NaN threshold and a negative threshold are refused with KSP_E_ARG.  Writes out_path (NULL / "":
 *   PREFIX_kSpider_dereplicated_<dist_type>.tsv) through .partial and a rename, on an error nothing is left behind:
 *   "source\trepresentative\t<dist_type>\tneighbours\trank", one row per source in .namesMap order: both names, the text of the
 *   assigning row's value exactly as it stands in the input ("-" for a representative), the degree, the rank.  Device =
 *   $KSPIDER_DEVICE (default 0); with $KSPIDER_VERBOSE one line reports records kept, representatives and rounds.
 * kspider_pairwise_and_dereplicate: kspider_pairwise's two TSVs, byte for byte, plus the same file, the selection taken from the
 *   gathered, sorted edges on the first device (the value text is ksp_format_float of the record's float).  The same refusals.
 *   At a threshold >= 0 a row that exists only with shared_kmers = 0 has the value 0 or NaN and never passes, so over the TSV
 *   kspider_pairwise wrote the two calls write the same bytes.  Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES.               */
#define KSP_DEREP_CHUNK_EDGES 2048u
#define KSP_DEREP_TAIL_PAIRS 65536u
int ksp_edges_dereplicate(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                          int dist_col, double threshold, uint32_t* h_rep, uint32_t* h_via, uint32_t* h_rank, uint32_t* h_degree,
                          uint32_t* n_reps);
int kspider_dereplicate(const char* index_prefix, const char* dist_type, double threshold, const char* out_path);
int kspider_pairwise_and_dereplicate(const char* index_prefix, int user_threads, const char* dist_type, double threshold,
                                     const char* out_path);

/* ---- top-k neighbours: each source's best hits, from the edges in HBM ----------------------------------------
 * The question asked first of a containment matrix: for this source, which are its closest ones, and how close?  The one
 * result that is bounded (n_nodes x k) however dense the graph is.
 * ENTRIES: an entry of node v is a record that names v and is no self pair (source_1 != source_2).  Every such record is an
 * entry of both of its ends, whatever its `shared`; a pair that repeats is listed again; a record naming a node >= n_nodes is
 * the caller's error and is ignored, as in ksp_components_edges.  ORDER of the entries of v: (1) value descending, (2) a NaN
 * below every number — a source without k-mers is never somebody's best hit; note that the tree above puts a NaN on TOP,
 * because a NaN row is kept at every cut-off: here the opposite is right — (3) ties by record index, lower first.  A strict
 * total order, so the result is unique.  VALUE: the float of column 3, 4 or 5 in single precision exactly as the pairwise
 * writer computes it; +inf is a number and sorts first.  RESULT: h_count[v] = min(k, entries of v); h_index[v * k + i] for
 * i < h_count[v] is the record index of the i-th entry in that order; every slot behind h_count[v] is 0xFFFFFFFF.
 * ksp_edges_topk: d_edges: `n_edges` ksp_edge records in DEVICE memory, in any order, never written; d_kmer_counts and dist_col
 *   (3 / 4 / 5) as for ksp_components_edges.  h_index (host, n_nodes x k entries) and h_count (host, n_nodes entries).
 *   KSP_E_ARG for k == 0 or k > KSP_TOPK_MAX_K, a NULL pointer with n_edges > 0, a NULL h_count (or h_index with n_nodes > 0)
 *   and a column other than 3 / 4 / 5; KSP_E_LIMIT for 2^32 - 1 records or more (the index is half of the 64-bit key and
 *   0xFFFFFFFF is "none") and, before anything is written to the caller, when
 *       16 * n_edges + (32 + 4 * k) * n_nodes + 64 bytes + the scratch of rocPRIM's scan over n_nodes + 1 values
 *   do not fit the device's free memory: one 8-byte key per entry and at most two entries per record; per node its number of
 *   entries (4), its 64-bit offset (8), its cursor (4), a slot in each of the three class lists (12), its count (4) and its k
 *   indices.  (ksp_topk_ranked: 12 bytes per edge more, for the uploaded edges.  KSP_TOPK_SELECT=library: 8 bytes per entry
 *   more, and the sort's scratch.)  Nothing is written to the caller's arrays unless the whole call succeeded.  n_edges = 0:
 *   all counts 0, all slots 0xFFFFFFFF, no kernel runs.  A node is selected by one of three kernels, by its number of entries
 *   n and nothing else: n <= KSP_TOPK_WAVE_ENTRIES by one wave, n <= KSP_TOPK_LDS_ENTRIES by one workgroup that sorts the
 *   segment in LDS (32 KiB, so that two workgroups fit a CU with room to spare), anything larger by one workgroup that keeps
 *   the best k in LDS and streams the segment through the other KSP_TOPK_LDS_ENTRIES - k slots.  $KSP_TOPK_MAX_WORKGROUPS
 *   caps every grid (tests); $KSP_TOPK_SELECT=library replaces the three kernels by rocPRIM's segmented radix sort (tests and
 *   timing: the same result; fewer than 2^32 - 1 entries), any other value than that, "kernels" or "" is KSP_E_ARG.
 *   KSP_TOPK_CHUNK_EDGES: records per chunk of the edge passes.  The class limits are UNMEASURED design choices: DESIGN.md 7j.
 * ksp_topk_ranked: the same selection for HOST edges whose values the caller has ranked: a higher h_rank is better, ties go to
 *   the lower index.  KSP_E_ARG for an endpoint >= n_nodes; the other refusals as above.  The same select kernels run.
 * kspider_topk: reads what kspider_tree reads, with the same validation and the same refusals (every row is an entry, so every
 *   row's ids must be rows of .namesMap), each before any file is written; "ani" goes through
 *   PREFIX_kSpider_pairwise.ani_col.tsv; dist_type NULL / "": "max_cont".  The weight of a row is its text read as a double, a
 *   NaN the lowest; the host sorts the distinct weights into ranks, the device selects.  Writes out_path (NULL / "":
 *   PREFIX_kSpider_topk_<dist_type>.tsv) through .partial and a rename, on an error nothing is left behind:
 *   "source\thit\tneighbour\t<dist_type>", one row per hit, the sources in .namesMap order and their hits 1, 2, ... in order:
 *   both names from .namesMap, the value as the text stands in the input.  A source without entries has no row.  KSP_E_ARG for
 *   k == 0, k > KSP_TOPK_MAX_K and an unknown distance.  Device = $KSPIDER_DEVICE (default 0); with $KSPIDER_VERBOSE one line
 *   reports the records, the hits written and the nodes per class.
 * kspider_pairwise_and_topk: kspider_pairwise's two TSVs, byte for byte, plus the same file, the selection taken from the
 *   gathered, sorted edges on the first device (the value text is ksp_format_float of the record's float).  Rows that exist
 *   only with shared_kmers = 0 (colours of weight 0) are merged in on the host by the same order, with their place in the
 *   (source_1, source_2) order of all rows as the index.  Every source of the index must be a row of .namesMap.  "ani" is
 *   refused with KSP_E_ARG, as in the sibling calls.  Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES.  This path orders by the
 *   FLOAT, which is finer than the 6-digit text kspider_topk reads, so among rows of equal text the two may choose or order
 *   differently.  Promised instead: per source both files have the same number of rows and the same column of value texts,
 *   line by line, and a row whose neighbour differs carries a value text that occurs more than once among that source's rows
 *   of the TSV (tests/test_topk_gpu.py::test_files).                                                                        */
#define KSP_TOPK_CHUNK_EDGES 2048u
#define KSP_TOPK_WAVE_ENTRIES 64u
#define KSP_TOPK_LDS_ENTRIES 4096u
#define KSP_TOPK_MAX_K 1024u
int ksp_edges_topk(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                   int dist_col, uint32_t k, uint32_t* h_index /* n_nodes x k */, uint32_t* h_count /* n_nodes */);
int ksp_topk_ranked(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const uint32_t* h_rank,
                    uint64_t n_edges, uint32_t k, uint32_t* h_index, uint32_t* h_count);
int kspider_topk(const char* index_prefix, const char* dist_type, uint32_t k, const char* out_path);
int kspider_pairwise_and_topk(const char* index_prefix, int user_threads, const char* dist_type, uint32_t k, const char* out_path);

/* ---- the cluster report: density, medoid and coverage of every cluster, from the edges in HBM ------------------
 * kspider_cluster says WHICH sources form a cluster; this says how good the cluster is and which member stands for it.  Single
 * linkage chains: a component may be a clique or a string of pairs that barely pass the cut-off, and only its edges tell.
 * Inputs as for ksp_components_edges: `n_edges` ksp_edge records in DEVICE memory, in any order, never written; d_kmer_counts;
 * dist_col 3 / 4 / 5; cutoff.
 * VALUE of a record: the float of the column in single precision exactly as the pairwise writer computes it.  A record is KEPT
 * when ksp_components_edges keeps it (the critical float of the reference's text test; a NaN is kept), both ends are < n_nodes
 * (a larger end is the caller's error and the record is ignored, as in the siblings) and source_1 != source_2 (a self pair takes
 * no part in anything).  A pair that repeats counts again; source_1 > source_2 is allowed.
 * CLUSTERS: the components of the kept records; label[v] = the smallest node of v's component, exactly the labels
 * ksp_components_edges returns.
 * DOMAIN: a containment lies in [0, 1].  A kept record whose value is not a NaN and exceeds 1 (+inf included: a count of 0
 * beside shared > 0) is refused with KSP_E_ARG: found on the device, nothing is written to the caller.
 * QUANTISED VALUE: q(v) = (uint64_t)((double)v * 4294967296.0), floor(v * 2^32): exact for v >= 2^-8, truncated below.  All sums
 * are sums of q in uint64_t, so every result is independent of record order, grid size and scheduling; with n_edges < 2^32 - 1
 * no sum can overflow.  A NaN record has no q.
 * PER NODE v: degree = the kept records naming v, NaN records included; strength = the sum of q over the others.
 * PER CLUSTER: size; edges = its kept records; nan_edges; sum_q; min / max over the values that are no NaN (both NaN when there
 * are none); medoid = the member of the largest strength, ties to the smallest node (a singleton is its own); covered = the
 * members other than the medoid that share a kept record with it.
 * via[v]: the lowest index of a kept record between v and the medoid of v's cluster; 0xFFFFFFFF for the medoid itself and for
 * members not adjacent to it.  covered = the members with a via.  Only via depends on the order of the records.
 * ksp_edges_cluster_report: h_cluster (host, room for n_nodes rows) receives *n_clusters rows in order of root, ascending; rows
 *   behind that are not written; h_member (host, n_nodes rows).  KSP_E_ARG for a NULL pointer with n_edges > 0, a NULL
 *   n_clusters (or h_cluster / h_member with n_nodes > 0), a column other than 3 / 4 / 5, a NaN cut-off and the domain refusal;
 *   KSP_E_LIMIT for 2^32 - 1 records or more (a record's index is `via`, and 0xFFFFFFFF is "none") and, before anything is
 *   written to the caller, when
 *       64 * n_nodes + 64 bytes
 *   do not fit the device's free memory: per node its label (4), degree (4), strength (8) and via (4), and in the slot of a
 *   root the cluster's edges, nan_edges and sum_q (8 each), min and max (4 each), the best strength (8) and the medoid (4); the
 *   flag, the round's scratch and the counters.  (ksp_cluster_report_valued: 12 bytes per edge more, for the uploaded edges.)
 *   Sizes, covered and the rows in root order are made by the host from those arrays.  Nothing is written to the caller unless
 *   the whole call succeeded.  n_edges = 0: every node is a singleton cluster, no kernel runs.  $KSP_REPORT_MAX_WORKGROUPS caps
 *   every grid (tests).  KSP_REPORT_CHUNK_EDGES: records per chunk and 256-thread workgroup of the edge passes, a design choice
 *   inherited from the cut (KSP_CUT_CHUNK_EDGES), not measured for this consumer.
 * ksp_cluster_report_valued: the same computation for HOST edges the caller has cut already: every record is kept (a self pair
 *   is still no part of anything), h_value may be NaN, a value above 1 is refused as above and so is one below 0; an end
 *   >= n_nodes is KSP_E_ARG.  The same kernels run behind an input adaptor.
 * kspider_cluster_report: reads what kspider_cluster reads, with the same validation and the same refusals, each before any file
 *   is written; a kept row's ids must be rows of .namesMap; the host applies kspider_cluster's test to the text as it stands, the
 *   value is that text read with strtof.  dist_type "min_cont", "avg_cont", "max_cont" (NULL / ""); "ani", a NaN cut-off and a
 *   cut-off outside [0, 1] are KSP_E_ARG.  Writes, through .partial and a rename (on an error nothing new is left behind),
 *   with <P> the text in the cluster file's name (cutoff * 100 as Python prints a float):
 *   PREFIX_kSpider_cluster_report_<dist_type>_<P>%.tsv: "cluster\tsize\tedges\tdensity\tmin\tmean\tmax\tmedoid\tmedoid_strength\tcovered",
 *     one row per cluster in the order of kspider_cluster's file, `cluster` the 1-based number of that file's line; density =
 *     edges / (size * (size - 1) / 2), mean = (double)sum_q / (double)(edges - nan_edges) / 2^32, medoid_strength = strength /
 *     2^32, all three "%.6g" and "-" where the divisor is 0; min / max as ksp_format_float prints them, "-" when NaN; medoid: a name.
 *   PREFIX_kSpider_cluster_members_<dist_type>_<P>%.tsv: "source\tcluster\tmedoid\t<dist_type>\tneighbours\tstrength", one row per
 *     source in .namesMap order: its name, its cluster's number, the medoid's name, the value text of the via row exactly as it
 *     stands in the input ("-" without one), degree, strength / 2^32 as "%.6g".
 *   Device = $KSPIDER_DEVICE; with $KSPIDER_VERBOSE one line reports the records kept, the clusters and the largest one's size and density.
 * kspider_pairwise_and_cluster_report: kspider_pairwise's two TSVs, byte for byte, plus the same two files, the report taken from
 *   the gathered, sorted edges on the first device (the value text of a via row is ksp_format_float of the record's float).
 *   Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES and with KSPIDER_TSV=device.  Rows that exist only with shared_kmers = 0 never
 *   reach the device; they are kept when they are NaN or when cutoff * 100 <= 0, and if at least one is kept the report is made
 *   by ksp_cluster_report_valued over ALL rows in (source_1, source_2) order, floats from the records: no such row is silently
 *   missing.  This path sums the FLOATS, which are finer than the 6-digit text kspider_cluster_report reads.  Promised against
 *   kspider_cluster_report over the TSV just written: the same clusters, sizes, edges, densities and min / max texts (six
 *   digits survive the trip through a float); where every value of the column has at most 6 significant decimal digits all
 *   four files are byte-equal; otherwise mean, the strengths and a medoid chosen among near-ties may differ (and with it
 *   covered and the via columns).                                                                                           */
typedef struct ksp_cluster_row {
    uint32_t root, size;
    uint64_t edges, nan_edges, sum_q;
    float min, max;
    uint32_t medoid, covered;
} ksp_cluster_row;   /* 48 bytes */
typedef struct ksp_member_row {
    uint32_t label, degree;
    uint64_t strength;
    uint32_t via, reserved /* 0 */;
} ksp_member_row;   /* 24 bytes */
#define KSP_REPORT_CHUNK_EDGES 2048u
int ksp_edges_cluster_report(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                             int dist_col, double cutoff, ksp_cluster_row* h_cluster /* room for n_nodes */, uint32_t* n_clusters,
                             ksp_member_row* h_member /* n_nodes */);
int ksp_cluster_report_valued(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const float* h_value,
                              uint64_t n_edges, ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member);
int kspider_cluster_report(const char* index_prefix, const char* dist_type, double cutoff);
int kspider_pairwise_and_cluster_report(const char* index_prefix, int user_threads, const char* dist_type, double cutoff);

/* ---- the average-linkage tree (UPGMA) of the containment graph, exact, from the edges in HBM (csrc/upgma.hip) -----
 * Single linkage chains; average linkage is what users of genome clustering reach for instead (dRep's secondary clustering,
 * scipy's linkage(..., 'average')).  Here it runs on the sparse edge list: no N x N matrix and no node limit.
 * RECORDS: inputs as for ksp_edges_cluster_report: `n_edges` ksp_edge records in DEVICE memory, any order, never written;
 * d_kmer_counts; dist_col 3 / 4 / 5.  The VALUE of a record is the float of the column exactly as the pairwise writer computes it.
 * q(v) = (uint64_t)((double)v * 4294967296.0), as in the report.  A record TAKES PART when both ends are < n_nodes (a larger end
 * is the caller's error and is ignored, as in the siblings), source_1 != source_2 and q > 0: a NaN, a 0 and a value below 2^-32
 * take no part, so a row that exists only with shared_kmers = 0 never matters.  A pair that repeats counts again; source_1 >
 * source_2 is allowed.  DOMAIN: a value that is not a NaN and exceeds 1 (+inf included), in a record whose ends are both nodes
 * (a self pair too), is refused with KSP_E_ARG: found on the device, nothing is written to the caller.
 * CLUSTERS: a cluster is named by its smallest member, its root.  S(A, B) = the sum of q over the participating records between a
 * member of A and a member of B.  {A, B} is a CANDIDATE when S(A, B) > 0; its similarity is the rational S(A, B) / (|A| * |B|),
 * in containment units that divided by 2^32.  Pairs without a record between them have similarity 0 and are never merged: the
 * result is a forest, like kspider_tree's.
 * ORDER of candidate pairs, a strict total order: similarity descending, compared exactly by cross-multiplication in 128 bits
 * (S < 2^64 because n_edges < 2^32 - 1 and q <= 2^32; |A| * |B| < 2^64; so a cross product is below 2^128); then the smaller
 * root ascending; then the larger root ascending.
 * RESULT: start from singletons and repeatedly merge the first candidate pair.  A merge is the row (lo, hi, sum_q = S, size_lo,
 * size_hi), lo < hi the two roots; the merged cluster's root is lo.  Rows are returned in merge order.  Average linkage is
 * reducible, so the rows are strictly descending in the order above and a cut at any similarity keeps a prefix of them.
 * The device computes it in rounds (every cluster picks its first candidate; pairs picked by both ends merge, all at once; the
 * rest is contracted), which gives exactly these rows: DESIGN.md 7m.  Rounds are at most n_nodes - 1; a path with monotone
 * weights needs about 0.6 * n_nodes of them.
 * ksp_edges_upgma: h_rows (host, room for n_nodes - 1 rows) receives *n_rows rows; rows behind that are not written.  KSP_E_ARG for
 *   a NULL pointer with n_edges > 0, a NULL n_rows, a NULL h_rows with n_nodes > 1, a column other than 3 / 4 / 5 and the domain
 *   refusal; KSP_E_LIMIT for 2^32 - 1 records or more (checked before any device call) and, before anything is written to the
 *   caller, when
 *       32 * n_edges + 16 * (ceil(n_edges / 2048) + 1) + 40 * n_nodes + 64 bytes
 *       + the larger of rocPRIM's scratch for the sort of n_edges (key, value) pairs of 8 + 8 bytes and for its scan of
 *         ceil(n_edges / 2048) + 1 counts
 *   do not fit the device's free memory: two (key, S) buffers of 16 bytes per record, the chunk counts and offsets, per node its
 *   size (4), map (4) and best (8) and a 24-byte row of the merge log, the counters.  KSP_E_HIP with a message, never a spin,
 *   should a round merge nothing while pairs are live or the rounds exceed n_nodes.  Nothing is written to the caller unless the
 *   whole call succeeded.  n_edges = 0 (or n_nodes < 2): *n_rows = 0, no kernel runs.  $KSP_UPGMA_MAX_WORKGROUPS caps every grid
 *   (tests).  KSP_UPGMA_CHUNK_EDGES: entries per chunk and 256-thread workgroup, inherited from the cut, not measured here.
 *   KSP_UPGMA_TAIL_PAIRS: at that many live pairs or fewer the pair list goes to the host, which finishes sequentially with the
 *   same comparison (the top of the tree merges a handful of big clusters one pair per round); $KSP_UPGMA_TAIL_PAIRS overrides
 *   it, 0 keeps the device rounds to the end; the rows are the same either way.  Measured on an MI355X (the table of DESIGN.md
 *   7m): on a path the host finish beats the device's rounds up to about 2^15 pairs, but on the bench workload's edges a
 *   hand-over above 1 024 pairs only costs, so the constant is the smaller figure.
 * ksp_upgma_valued: the same for HOST edges the caller has valued already; the same kernels run behind an input adaptor.  An end
 *   >= n_nodes, a value below 0 and a value above 1 are KSP_E_ARG; a NaN takes no part.  (12 bytes per edge more.)
 * ksp_upgma_before: host only — the comparison of two pairs: *before = 1 when the first comes first in the order, else 0.
 *   KSP_E_ARG for a NULL pointer and a size of 0.
 * kspider_upgma: reads what kspider_tree reads, with the same validation and refusals, each before any file is written; the ids of
 *   a participating row must be rows of .namesMap; the value is the column's text read with strtof.  dist_type "min_cont",
 *   "avg_cont", "max_cont" (NULL / ""); "ani" and an unknown distance are KSP_E_ARG.  Writes, through .partial and a rename,
 *   PREFIX_kSpider_upgma_<dist>.tsv: "source_1\tsource_2\t<dist>_average\tsum_q\tsize_1\tsize_2\tmerged_size", one row per merge in
 *   merge order, the two ids the .namesMap ids of lo and hi, the average (double)sum_q / ((double)size_1 * size_2) / 2^32 as
 *   "%.9g" (for people: sum_q and the sizes, decimal, are the exact data).  newick != 0: also PREFIX_kSpider_upgma_<dist>.newick by
 *   the conventions of kspider_tree's: height of a merge 1 - average clamped to [0, 1], branch lengths "%.6g", the child holding
 *   lo first, clusters that never join under one root at height 1 in order of their smallest node, a single node `name;`.
 *   Device = $KSPIDER_DEVICE; with $KSPIDER_VERBOSE one line reports the records taking part, the pairs, the device rounds and the
 *   merges made on the device / by the host finish.
 * kspider_cluster_from_upgma: host only — reads .namesMap and that merge table and keeps a row when sum_q >= q_cut * size_1 *
 *   size_2 in 128 bits, q_cut = (uint64_t)(cutoff * 4294967296.0); writes PREFIX_kSpider_clusters_upgma_<dist>_<P>%.tsv, P =
 *   cutoff * 100 as Python prints a float, in the format and order kspider_cluster uses.  KSP_E_ARG for a cut-off outside [0, 1]
 *   or NaN and an unknown distance; KSP_E_IO for a missing or malformed table or an id that is not in .namesMap.
 * kspider_pairwise_and_upgma: kspider_pairwise's two TSVs, byte for byte, plus the files of kspider_upgma, the tree taken from the
 *   gathered, sorted edges on the first device.  Works with $KSPIDER_DEVICE / $KSPIDER_DEVICES and with KSPIDER_TSV=device.  Rows
 *   that exist only with shared_kmers = 0 have q = 0 and need no host merge.  Every source of the index must be a row of
 *   .namesMap.  This path sums the FLOATS, kspider_upgma the 6-digit texts: where every value of the column has at most 6
 *   significant decimal digits all files are byte-equal; otherwise sums, averages and choices among near-ties may differ.   */
typedef struct ksp_upgma_row {
    uint32_t lo, hi;
    uint64_t sum_q;
    uint32_t size_lo, size_hi;
} ksp_upgma_row;   /* 24 bytes */
#define KSP_UPGMA_CHUNK_EDGES 2048u
#define KSP_UPGMA_TAIL_PAIRS 1024u   /* measured: DESIGN.md 7m */
int ksp_edges_upgma(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                    int dist_col, ksp_upgma_row* h_rows /* room for n_nodes - 1 */, uint32_t* n_rows);
int ksp_upgma_valued(int device, uint32_t n_nodes, const uint32_t* h_a, const uint32_t* h_b, const float* h_value, uint64_t n_edges,
                     ksp_upgma_row* h_rows, uint32_t* n_rows);
int ksp_upgma_before(uint64_t s1, uint32_t size_lo1, uint32_t size_hi1, uint32_t lo1, uint32_t hi1,
                     uint64_t s2, uint32_t size_lo2, uint32_t size_hi2, uint32_t lo2, uint32_t hi2, int* before);
int kspider_upgma(const char* index_prefix, const char* dist_type, int newick);
int kspider_pairwise_and_upgma(const char* index_prefix, int user_threads, const char* dist_type, int newick);
int kspider_cluster_from_upgma(const char* index_prefix, const char* dist_type, double cutoff);

/* ---- the rows of the pairwise TSV as text, made on the device (csrc/tsv.hip) ----
 * ksp_edges_tsv: the text of `n_edges` ksp_edge records in DEVICE memory (never written), in their order, rows only, no header:
 *       id1 \t id2 \t shared \t min \t avg \t max \n
 *   byte for byte what the pairwise writer prints for the record: id = d_ids[source] (device, n_nodes entries), or the source
 *   index itself when d_ids is NULL; shared in decimal; the three containments in the writer's single-precision maths from
 *   d_kmer_counts (device, n_nodes entries), each as `std::ostream << float` prints it (ksp_format_float, "%.6g"): the digits come
 *   from integer arithmetic on the float's exact binary value, rounded to nearest, ties to even (csrc/tsv_text.h).
 *   *n_bytes = the bytes of the text.  h_text NULL: the size query, nothing is written.  capacity < *n_bytes: KSP_E_OVERFLOW,
 *   *n_bytes is set and nothing is written.  Otherwise h_text (host) receives exactly *n_bytes bytes, no terminator.  A row is
 *   KSP_TSV_ROW_MIN = 12 to KSP_TSV_ROW_MAX = 79 bytes (two ids of 10 digits, a count of 20, three floats of 11, six
 *   separators), so 79 * n_edges always suffices; byte counts and offsets are 64-bit throughout.  n_edges = 0: 0 bytes, no
 *   kernel runs.  KSP_E_ARG, with nothing written, for a NULL d_kmer_counts or n_bytes, a NULL d_edges with n_edges > 0, and
 *   — found on the device — a record naming a source >= n_nodes, a row with a NaN column (shared = 0 beside a count of 0: its
 *   text is the host libc's business) and a column outside the formatter's domain: 0, +inf and the positive floats in
 *   [2^-40, 2^40) (no record with counts and sums below 2^32 leaves it).  Rows are taken in chunks of KSP_TSV_CHUNK_ROWS;
 *   the text leaves the device through a window in HBM and from there in pieces of $KSP_TSV_PIECE bytes (default 8 MiB;
 *   tests: any size >= 1, pieces end inside rows) through two pinned staging buffers, as ksp_engine_join_to_host moves edges.
 *   $KSP_TSV_MAX_WORKGROUPS caps the grids (tests).  $KSPIDER_TSV=device makes the drop-in calls (kspider_pairwise and its
 *   _cut / _and_* siblings over an index) write PREFIX_kSpider_pairwise.tsv from this text: the same bytes, see DESIGN.md 7k. */
#define KSP_TSV_CHUNK_ROWS 256u
int ksp_edges_tsv(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts,
                  const uint32_t* d_ids, char* h_text, uint64_t capacity, uint64_t* n_bytes);

/* ---- query mode: new sketches against a database, without the N x N join (csrc/query.hip, csrc/sketch_pack.cpp) ----
 * Numbering: database sources are 0 .. n_db - 1, queries n_db .. n_db + n_q - 1.  An edge is a ksp_edge with source_1 < source_2 in
 * that numbering and shared > 0.  mode KSP_QUERY_CROSS: only database x query pairs (source_1 < n_db <= source_2);
 * KSP_QUERY_CROSS_AND_SELF: also every query x query pair once (source_2 >= n_db) — the old database x database table plus this
 * result is the full table of the union (the append case).  Runs are duplicate-free within a source, as everywhere in this ABI;
 * the table build sorts and deduplicates the query side itself, and the probe does not depend on the order of a database run.
 * ksp_query_device: the caller keeps the database in HBM and calls per batch of queries.  d_db_keys / d_q_keys: DEVICE memory, the
 *   runs back to back; h_db_offsets / h_q_offsets: HOST memory, n + 1 element offsets.  The edges go to d_edges (device, room for
 *   `capacity` records) in unspecified order; *n_edges = the edges found.  More than `capacity`: KSP_E_OVERFLOW, *n_edges is the
 *   required size and nothing was written past `capacity`; d_edges NULL with capacity 0 is the size query.  KSP_E_ARG, before
 *   anything is allocated: a NULL pointer (stats may be NULL), n_db = 0 or n_q = 0, offsets that do not start at 0 or decrease, an
 *   unknown mode.  KSP_E_LIMIT: n_db + n_q > 2^32 - 2, a query tile of 2^31 entries or more, memory that does not fit the device's
 *   free memory (the message says what was asked).  The queries are taken in tiles of at most KSP_QUERY_TILE_MAX: n_q above it
 *   means one pass over the database per tile.  Read on every call: $KSP_QUERY_TILE (queries per tile, 1 .. KSP_QUERY_TILE_MAX),
 *   $KSP_QUERY_LONG_RUN (a probe source of that many entries or more gets a workgroup instead of a wave; default
 *   KSP_QUERY_LONG_RUN), $KSP_QUERY_LIST (touched-list capacity, 1 .. KSP_QUERY_LIST_MAX), $KSP_QUERY_MAX_WORKGROUPS (caps the grids;
 *   tests).  The result is the same under each.
 * ksp_query_host: the same for HOST arrays: uploads, calls, retries once at the exact size, sorts the edges by (source_1, source_2)
 *   on the device and returns them in *edges (ksp_free).  A device that is not there: KSP_E_HIP, "ksp_query_host: no such device".
 * ksp_query_directory: host only — the first level of a tile's table: for a table of n_keys distinct keys, the largest max_key,
 *   dir[b] is the first index whose key >> *shift is >= b, b = 0 .. 2^*bits.  *bits + *shift = the significant bits of max_key;
 *   about four keys per bucket of a uniform table, 1 <= *bits <= KSP_QUERY_DIR_BITS_MAX (0 and shift 0 for max_key = 0).
 * kspider_pack: one pack file (csrc/sketch_set.h: little-endian, fixed width) from a directory of .sig / .gz files (kSize > 0) or
 *   .bin files (kSize = 0); group ids, names, k-mer counts and the skipping of a signature without that ksize are exactly those of
 *   kspider_pairwise_sigs / kspider_pairwise_bins.  Written through OUT.partial and a rename: a failed write leaves no file.
 * ksp_pack_info / ksp_pack_load: host only — read a pack file whole and checked, or refuse with KSP_E_IO and nothing written to the
 *   caller: a wrong magic or version, a length that is not exactly what the header implies, offsets that do not start at 0 or
 *   decrease, a run that is not strictly ascending, a presence or name count that disagrees with the header.  out[0] kSize, out[1]
 *   groups G, out[2] groups with a sketch S, out[3] keys K, out[4] bytes of all names B.  load: kmers[G], present[G], offsets[S + 1],
 *   keys[K], name_offsets[G + 1], names[B] (no terminators).
 * kspider_query: db and queries are each a pack file or a directory (.sig / .gz for kSize > 0, .bin for kSize = 0); a pack whose
 *   kSize differs from a non-zero kSize is KSP_E_ARG; out_prefix is required.  Writes OUT.namesMap (database names with ids 1 .. N,
 *   then the queries N + 1 .. N + Q), OUT_kSpider_seqToKmersNo.tsv and OUT_kSpider_pairwise.tsv with only the rows of the mode,
 *   sorted by (source_1, source_2), maths and text those of the pairwise writer — ordinary pairwise files for kspider_topk,
 *   kspider_cluster, kspider_export and the others.  A refused or failed call writes no file.  Device = $KSPIDER_DEVICE (default
 *   0); $KSPIDER_DEVICES and $KSPIDER_TSV are not read.                                                                          */
#define KSP_QUERY_CROSS 0
#define KSP_QUERY_CROSS_AND_SELF 1
#define KSP_QUERY_TILE_MAX 2048u      /* 8 KiB of u32 counters per probe source in LDS */
#define KSP_QUERY_LIST_MAX 512u
#define KSP_QUERY_LONG_RUN 2048u
#define KSP_QUERY_DIR_BITS_MAX 24
typedef struct ksp_query_stats {
    uint64_t n_db, n_q;
    uint64_t db_entries, q_entries;
    uint64_t table_keys;       /* distinct keys, summed over the tiles                                  */
    uint64_t table_holders;    /* (key, query) memberships, summed over the tiles                      */
    uint64_t passes;           /* query tiles probed: passes over the database                         */
    uint64_t short_sources;    /* probe sources of a pass that get a wave                              */
    uint64_t long_sources;     /* ... that get a workgroup                                             */
    uint64_t list_overflows;   /* (source, tile) emissions that scanned all counters                   */
    uint64_t edges;
    uint64_t long_run;         /* the switches as the call read them                                   */
    float ms_table, ms_probe;  /* HIP-event times, summed over the tiles                               */
    float ms_sort;             /* ksp_query_host: the sort of the edges                                */
    uint32_t tile, list_capacity, reserved;
} ksp_query_stats;   /* 120 bytes */
int ksp_query_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys,
                     const uint64_t* h_q_offsets, uint32_t n_q, int mode, ksp_edge* d_edges, uint64_t capacity, uint64_t* n_edges,
                     ksp_query_stats* stats);
int ksp_query_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint64_t* q_offsets,
                   uint32_t n_q, int mode, int device, ksp_edge** edges, uint64_t* n_edges, ksp_query_stats* stats);
int ksp_query_directory(uint64_t max_key, uint64_t n_keys, int* bits, int* shift);
int kspider_pack(const char* dir, int kSize, const char* out_path, int user_threads);
int ksp_pack_info(const char* path, uint64_t out[5]);
int ksp_pack_load(const char* path, uint32_t* kmers, uint8_t* present, uint64_t* offsets, uint64_t* keys, uint64_t* name_offsets, char* names);
int kspider_query(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, int mode);

/* ---- gather: what is each query made of?  The greedy minimum-set-cover by database sources (csrc/gather.hip) ----
 * Database sources are 0 .. n_db - 1, queries 0 .. n_q - 1, each a strictly ascending run of 64-bit hashes as in ksp_query_*.
 * Every query q with hash set Q is treated on its own:  R = Q, rank = 0;  loop: u(s) = |S_s ∩ R| for every source s; s* = the
 * source with the largest u, among equals the smallest s; stop when u(s*) < min_hashes, or when max_matches is not 0 and rank has
 * reached it; otherwise rank += 1, R = R \ S_s*, and the row is (q, rank, s*, overlap = |S_s* ∩ Q|, unique = u(s*),
 * remaining = |R|).  Rows are ordered by (query, rank); everything is an integer and the tie rule is total, so the table is the
 * same under every switch and schedule.
 * ksp_gather_device: the caller keeps the database in HBM across calls.  d_db_keys / d_q_keys: DEVICE memory, the runs back to
 *   back; h_db_offsets / h_q_offsets: HOST memory, n + 1 element offsets.  The rows go to d_rows (device, room for `capacity`);
 *   *n_rows = the rows found.  More than `capacity`: KSP_E_OVERFLOW, *n_rows is the required size, the first `capacity` rows were
 *   written and nothing past them; d_rows NULL with capacity 0 is the size query.  KSP_E_ARG, before a device is chosen and before
 *   anything is allocated: a NULL pointer (stats may be NULL), d_rows NULL with a capacity, n_db = 0 or n_q = 0, min_hashes = 0,
 *   offsets that do not start at 0 or decrease, a switch of the environment that is not a number in its range.  KSP_E_LIMIT:
 *   n_db + n_q > 2^32 - 2, a query tile of 2^31 entries or more, 2^32 - 1 or more candidates or matched hashes of candidates in
 *   one query tile, memory that does not fit the device's free memory (the message says what was asked: beside query mode's table,
 *   40 bytes per candidate — a (source, query) pair with overlap >= min_hashes —, 4 per matched hash of a candidate, a bit per
 *   query hash, 48 per possible row).  The queries are taken in tiles as in query mode: one pass over the database per tile, and a
 *   second over the sources that have a candidate.  Read on every call: $KSP_QUERY_TILE, $KSP_QUERY_LONG_RUN, $KSP_QUERY_LIST as in
 *   query mode; $KSP_GATHER_LONG_SEG (a candidate of that many matched hashes or more is counted by a workgroup instead of a wave;
 *   1 .. 2^32 - 1, default KSP_GATHER_LONG_SEG); $KSP_GATHER_TAIL (0: rounds in batches to the end; 1, the default: one workgroup
 *   runs the remaining rounds once at most $KSP_GATHER_TAIL_CANDS candidates are live, 0 .. KSP_GATHER_TAIL_CANDS_MAX, default
 *   KSP_GATHER_TAIL_CANDS); $KSP_GATHER_MAX_WORKGROUPS (caps the grids; tests).  The rows are the same under each.  Rounds are
 *   launched KSP_GATHER_BATCH at a time; the host reads the device's count of live queries once per batch.
 * ksp_gather_host: the same for HOST arrays; the rows come back in *rows (ksp_free).  A device that is not there: KSP_E_HIP,
 *   "ksp_gather_host: no such device".
 * kspider_gather: db and queries are each a pack file or a directory, exactly as kspider_query loads them; out_prefix is required.
 *   Writes OUT_kSpider_gather.tsv: a header line, then per row the query's name, rank, the match's name, overlap, unique,
 *   f_orig_query = overlap / |Q|, f_unique_to_query = unique / |Q|, f_match = overlap / |S| (single precision, printed as
 *   ksp_format_float prints) and remaining.  The file is written through OUT.partial only after the call has succeeded: a refused
 *   or failed call writes none.  KSP_E_ARG: a NULL or empty argument, kSize < 0, min_hashes = 0, a pack of another kSize, a side
 *   without a sketch.  Device = $KSPIDER_DEVICE (default 0).                                                                      */
#define KSP_GATHER_BATCH 16u
#define KSP_GATHER_LONG_SEG 1024u
#define KSP_GATHER_TAIL_CANDS 256u
#define KSP_GATHER_TAIL_CANDS_MAX 1048576u
#define KSP_GATHER_FIRST_CANDS 4096u   /* candidates the first buffer of a call holds (or 4 per source); a tile with more is swept twice */
typedef struct ksp_gather_row {
    uint32_t query, rank, source;
    uint32_t overlap, unique, remaining;
} ksp_gather_row;   /* 24 bytes */
typedef struct ksp_gather_stats {
    uint64_t n_db, n_q;
    uint64_t db_entries, q_entries;
    uint64_t table_keys, table_holders;   /* as in ksp_query_stats, summed over the tiles                    */
    uint64_t passes;           /* query tiles swept: passes over the database                                */
    uint64_t candidates;       /* (source, query) pairs with overlap >= min_hashes                            */
    uint64_t dropped;          /* pairs with 0 < overlap < min_hashes: dropped before the rounds             */
    uint64_t fell_below;       /* candidates counted below min_hashes in a round: dead from then on          */
    uint64_t slots;            /* matched hashes of the candidates: u32 words of segments                    */
    uint64_t rounds;           /* rounds with a live query, summed over the tiles                            */
    uint64_t batches;          /* batches of KSP_GATHER_BATCH rounds launched = reads of the live count      */
    uint64_t tail_rounds;      /* of `rounds`, those the one-workgroup tail ran                              */
    uint64_t live_at_tail;     /* live candidates handed to the tail                                         */
    uint64_t rows;
    uint64_t long_seg;         /* the switches as the call read them                                         */
    uint64_t tail_cands;       /* (0 also when $KSP_GATHER_TAIL is 0)                                        */
    float ms_table, ms_candidates, ms_fill, ms_rounds;   /* HIP-event times, summed over the tiles           */
    uint32_t tile, min_hashes, max_matches, reserved;
} ksp_gather_stats;   /* 176 bytes */
int ksp_gather_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys,
                      const uint64_t* h_q_offsets, uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, ksp_gather_row* d_rows,
                      uint64_t capacity, uint64_t* n_rows, ksp_gather_stats* stats);
int ksp_gather_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint64_t* q_offsets,
                    uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, int device, ksp_gather_row** rows, uint64_t* n_rows,
                    ksp_gather_stats* stats);
int kspider_gather(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, uint32_t min_hashes,
                   uint32_t max_matches);

/* ---- weighted gather: the same decomposition of queries that carry an abundance per hash (csrc/gather.hip) ----
 * Query q has hash set Q and abundances a(h), uint32_t, parallel to its keys: q_abund[i] belongs to q_keys[i].  0 is legal and
 * counts as 0.  W = Σ_{h∈Q} a(h).  The greedy is exactly the one above — selection by the unweighted u(s), ties to the smaller
 * source, the same stops —, so the first six fields of every row are ksp_gather_*'s.  For the row of rank r let T = S_s* ∩ R
 * BEFORE the removal, n = |T| = unique.  The row additionally carries
 *   w_unique = Σ_{h∈T} a(h);   w_found = Σ of w_unique over ranks 1 .. r of this query;   sq_lo, sq_hi = the 128-bit Σ_{h∈T} a(h)²;
 *   median2 = a_(⌈n/2⌉) + a_(⌊n/2⌋+1) of T's abundances in ascending order (1-based): twice the median.
 * The statistics are over the hashes TAKEN IN THAT ROUND, with the original query's abundances — not over the whole overlap.
 * Everything is an integer, so the table is the same under every switch and schedule.  A database has no abundances here.
 * (A query that lists a hash more than once holds it once, as above, with the largest of the abundances listed for it.)
 * ksp_gather_abund_device / ksp_gather_abund_host: ksp_gather_device / ksp_gather_host with d_q_abund (DEVICE) / q_abund (HOST)
 *   beside the query keys and rows of ksp_gather_wrow.  The same argument, limit and overflow rules (q_abund NULL: KSP_E_ARG), the
 *   same switches, the same ksp_gather_stats.  Memory beside the unweighted call's: 4 bytes per holder of a tile's query table
 *   (the abundance at its holder slot), 8 per query of a tile, and 128 instead of 48 per possible row; the message names them.
 *   On the device: after a tile's table is built one pass puts a(h) at its holder slot; the take sums a and a² over the winner's
 *   alive slots before it clears them, compacts their abundances into the winner's own segment (dead after the take) and selects
 *   the median there: by ranking in registers up to 64 values, above by a radix select over 8-bit digits (a 256-bin histogram per
 *   wave in LDS, four passes).  One wave per take, as in the unweighted call; no library sort.
 * kspider_gather_abund: kspider_gather for queries that carry abundances.  `queries` must be a directory of signatures that all
 *   have "abundances": a pack file, or a signature without them, is KSP_E_ARG naming it.  Abundances of the database are
 *   ignored.  Writes OUT_kSpider_gather.tsv: kspider_gather's nine columns, byte for byte, then f_unique_weighted = w_unique / W,
 *   average_abund = w_unique / unique, median_abund = median2 / 2, std_abund = sqrt(n·sq − w_unique²) / n (the numerator exact
 *   in 128 bits, rounded once to double) — each cast to float and printed as ksp_format_float prints —, then the integers
 *   n_unique_weighted_found = w_unique, sum_weighted_found = w_found and total_weighted_hashes = W.  A refused or failed call
 *   writes no file.                                                                                                            */
typedef struct ksp_gather_wrow {
    uint32_t query, rank, source, overlap, unique, remaining;
    uint64_t w_unique, w_found, sq_lo, sq_hi, median2;
} ksp_gather_wrow;   /* 64 bytes */
int ksp_gather_abund_device(int device, const uint64_t* d_db_keys, const uint64_t* h_db_offsets, uint32_t n_db, const uint64_t* d_q_keys,
                            const uint32_t* d_q_abund, const uint64_t* h_q_offsets, uint32_t n_q, uint32_t min_hashes, uint32_t max_matches,
                            ksp_gather_wrow* d_rows, uint64_t capacity, uint64_t* n_rows, ksp_gather_stats* stats);
int ksp_gather_abund_host(const uint64_t* db_keys, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys, const uint32_t* q_abund,
                          const uint64_t* q_offsets, uint32_t n_q, uint32_t min_hashes, uint32_t max_matches, int device,
                          ksp_gather_wrow** rows, uint64_t* n_rows, ksp_gather_stats* stats);
int kspider_gather_abund(const char* db, const char* queries, int kSize, const char* out_prefix, int user_threads, uint32_t min_hashes,
                         uint32_t max_matches);

/* ---- sketching: FASTA / FASTQ in, sourmash-compatible DNA FracMinHash sketches out (csrc/sketch_hash.h, csrc/sketcher.hip,
 *      csrc/sketch_cpu.cpp, csrc/fastx_reader.cpp, csrc/sketch_files.cpp) ----
 * The definition.  Bytes ACGTacgt are bases, lower case counts as upper case; every other byte value breaks k-mers.  A k-mer is
 * ksize (1 .. 64) consecutive bases inside one source; its canonical form is the smaller, as text, of its upper-case letters and
 * their reverse complement; its hash is the first word of MurmurHash3_x64_128 over the ksize letters of the canonical form with
 * `seed` (sourmash: 42); it is kept iff hash <= max_hash.  A source's sketch is the ascending list of its distinct kept hashes.
 * The input of the compute calls is a byte stream and src_offsets[n_sources + 1] (ascending from 0 to n_bytes): source s is the
 * bytes [src_offsets[s], src_offsets[s + 1]).  Records inside a source are separated by any non-base byte.
 * ksp_sketch_max_hash: host only — sourmash's threshold of `scaled`: 2^64 - 1 for 1, (uint64_t)(2^64 / (double)scaled) above;
 *   KSP_E_ARG for 0.
 * ksp_murmur64: host only — both words of MurmurHash3_x64_128 over any bytes (data may be NULL with len 0).
 * ksp_sketch_kmer_hash: host only — the hash of the k-mer spelled by `ksize` bytes of text; *valid = 0 (and *hash = 0) when a
 *   byte is not a base.
 * ksp_sketch_cpu: host only — the plain single-thread loop: out_keys (room for `capacity`) receives the sketches back to back,
 *   out_offsets[n_sources + 1] their bounds, *needed = the keys of all sketches.  More than `capacity`: KSP_E_OVERFLOW with
 *   *needed and the offsets set and nothing written to out_keys; out_keys NULL with capacity 0 is the size query.
 * ksp_sketch_device: d_seq (16-byte aligned) and d_out_keys (room for `capacity`) are DEVICE memory, the offsets are on the
 *   host.  `capacity` must hold the survivors — the kept k-mers before duplicates are dropped —, whose number comes back in
 *   stats->needed: more than `capacity` is KSP_E_OVERFLOW, with stats->needed exact and nothing written to d_out_keys or
 *   h_out_offsets; d_out_keys NULL with capacity 0 is the size query.  One hash pass over the bytes (workgroups of 256 loop over
 *   tiles of KSP_SKETCH_TILE_BASES positions; $KSPIDER_SKETCH_MAX_WGS caps the grid), then the select pass: survivors sorted by
 *   (source, hash), adjacent duplicates dropped, per-source offsets.  The result does not depend on scheduling.  Takes max_hash,
 *   not scaled, so that the threshold can be tested at an exact value.  KSP_E_ARG, before a device is chosen: a NULL pointer,
 *   ksize outside 1 .. 64, n_sources = 0, offsets that do not start at 0, decrease or do not end at n_bytes, a d_seq that is not
 *   16-byte aligned.  KSP_E_LIMIT when the memory asked for (40 bytes per survivor of `capacity`, the sort's scratch, 16 per
 *   source) does not fit the device's free memory; nothing has run then.
 * ksp_sketch_host: the same for HOST arrays: uploads, calls, retries once at the exact size on overflow, and returns the keys in
 *   *out_keys (ksp_free).  $KSPIDER_SKETCH_FIRST_CAPACITY: the first call's capacity (tests: forces the retry).  A device that is
 *   not there: KSP_E_HIP, "ksp_sketch_host: no such device".
 * ksp_fastx_info / ksp_fastx_load: host only, two calls — the FASTA / FASTQ reader (plain or gzip; wrapped lines, CRLF, empty
 *   records, a missing final newline; FASTQ by its 4-line structure).  info: out[0] records, out[1] bytes of seq, out[2] bytes of
 *   the names, out[3] 0 FASTA / 1 FASTQ.  load: seq = every record's bases as they stand in the file followed by one '\n',
 *   rec_offsets[records + 1] their bounds, names = every header's first word back to back, name_offsets[records + 1].  KSP_E_IO,
 *   naming the file and the line, for a file that is neither, a FASTQ record cut short or with a quality line of another length,
 *   and a truncated or corrupt gzip.
 * kspider_sketch: the file driver.  input: a directory (its files ending in .fa .fasta .fna .fq .fastq, each optionally .gz, in
 *   the glob order of the sig loader, each one source named by the file without those endings), or one file, whose records are
 *   each a source named by the header's first word with KSP_SKETCH_PER_RECORD in flags and one source otherwise.  Writes
 *   out_dir/<name>.sig per source (out_dir is created): the fields of a sourmash signature file with one signature {num 0, ksize,
 *   seed, max_hash, molecule "DNA", md5sum, mins}; md5sum is the MD5 of the decimal text of ksize followed by the decimal text of
 *   every min, without separators.  seed: flags >> 32 when KSP_SKETCH_SEED is set, else 42.  Files are read by user_threads
 *   threads and sent in batches of at most $KSPIDER_SKETCH_BATCH_MB (256; $KSPIDER_SKETCH_BATCH_BYTES: the same in bytes, at
 *   least 1024) through pinned staging, the next batch being read while the device hashes; a source may span batches, a record
 *   longer than a batch is cut with ksize - 1 bytes of overlap, and the result does not depend on the batch size.
 *   KSPIDER_SKETCH=host runs the same driver over ksp_sketch_cpu: the same bytes, no GPU.  Works with $KSPIDER_DEVICE.
 *   KSP_E_ARG: NULL or empty input / out_dir, ksize outside 1 .. 64, scaled = 0, two sources of one name; KSP_E_IO: no input
 *   file, a reader error, a file that cannot be written.
 * Counted sketches.  With the definition above unchanged, the abundance of a kept hash in a source is the number of valid windows
 *   inside that source whose canonical k-mer has that hash: forward and reverse-complement occurrences count together.  It is
 *   clamped at 2^32 - 1 and is a uint32_t array parallel to the keys: abund[i] belongs to keys[i].
 * ksp_sketch_cpu_abund / ksp_sketch_device_abund / ksp_sketch_host_abund: the calls above with out_abund / d_out_abund / *out_abund
 *   (room for `capacity`; ksp_free for the host call's) beside the keys; the keys and offsets are those of the calls above, and
 *   the overflow, size-query, argument and limit rules are the same (out_abund NULL with a capacity: KSP_E_ARG; the device call
 *   asks for the same memory).  On the device the select pass's head of a run of equal (source, hash) entries writes
 *   min(the next head's index - its own, 2^32 - 1) beside its hash.
 * kspider_sketch with KSP_SKETCH_ABUND in flags: every signature has "abundances":[...] directly after "mins", parallel to it;
 *   md5sum is unchanged (sourmash's ignores abundances).  A source's sketch is the union of its segments' sketches WITH THE
 *   COUNTS ADDED (every window lies in exactly one piece of a cut record), clamped after adding; KSPIDER_SKETCH=host writes the
 *   same bytes.  Without the flag the files are what they were.
 * ksp_sig_read: host only — one .sig / .sig.gz file as the loaders read it: the first signature of that kSize; mins sorted,
 *   a hash listed twice once, with its abundances added and clamped; *has_abund = 1 when the signature has "abundances" (else
 *   abunds is untouched and may be NULL).  *n = the distinct mins.  More than `capacity`: KSP_E_OVERFLOW with *n set; mins NULL
 *   with capacity 0 is the size query.  KSP_E_IO naming the file: unreadable, malformed, no signature of that kSize, or
 *   "abundances" of another length than "mins".                                                                              */
#define KSP_SKETCH_TILE_BASES 4096u
#define KSP_SKETCH_PER_RECORD 1ull
#define KSP_SKETCH_SEED 2ull
#define KSP_SKETCH_ABUND 4ull
typedef struct ksp_sketch_stats {
    uint64_t bases;            /* base bytes of the stream                                                        */
    uint64_t valid_kmers;      /* windows of ksize bases without a break byte (one over a source boundary that no
                                  break byte marks is counted here and dropped when it is attributed)              */
    uint64_t kept;             /* survivors: windows with hash <= max_hash that lie inside a source                */
    uint64_t distinct_out;     /* keys of all sketches                                                            */
    uint64_t needed;           /* the capacity the call needs: = kept                                             */
    uint64_t workgroups;       /* the hash pass's grid                                                            */
    uint64_t retries;          /* ksp_sketch_host: 1 when the first capacity overflowed                           */
    float ms_upload, ms_hash, ms_select;   /* HIP-event times (upload: ksp_sketch_host only)                       */
    uint32_t reserved;
} ksp_sketch_stats;   /* 72 bytes */
int ksp_sketch_max_hash(uint64_t scaled, uint64_t* out);
int ksp_murmur64(const void* data, uint64_t len, uint32_t seed, uint64_t out[2]);
int ksp_sketch_kmer_hash(const char* text, int ksize, uint32_t seed, uint64_t* hash, int* valid);
int ksp_sketch_cpu(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, uint64_t max_hash,
                   uint32_t seed, uint64_t* out_keys, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed);
int ksp_sketch_device(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize,
                      uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint64_t capacity, uint64_t* h_out_offsets,
                      ksp_sketch_stats* stats);
int ksp_sketch_host(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize,
                    uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint64_t* out_offsets, ksp_sketch_stats* stats);
int ksp_fastx_info(const char* path, uint64_t out[4]);
int ksp_fastx_load(const char* path, uint8_t* seq, uint64_t* rec_offsets, uint64_t* name_offsets, char* names);
int kspider_sketch(const char* input, int kSize, uint64_t scaled, const char* out_dir, int user_threads, uint64_t flags);
int ksp_sketch_cpu_abund(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, uint64_t max_hash,
                         uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed);
int ksp_sketch_device_abund(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize,
                            uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint32_t* d_out_abund, uint64_t capacity,
                            uint64_t* h_out_offsets, ksp_sketch_stats* stats);
int ksp_sketch_host_abund(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize,
                          uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint32_t** out_abund, uint64_t* out_offsets,
                          ksp_sketch_stats* stats);
int ksp_sig_read(const char* path, int kSize, uint64_t* mins, uint32_t* abunds, uint64_t capacity, uint64_t* n, int* has_abund);

/* ---- protein, dayhoff and hp sketches; six-frame translation (csrc/sketch_mol.h, csrc/sketch_kernels.hip.h) ----
 * Molecule types: KSP_MOL_DNA 0 is the section above, untouched; KSP_MOL_PROTEIN 1, KSP_MOL_DAYHOFF 2, KSP_MOL_HP 3.
 * Residues.  A residue byte is an ASCII letter (either case, taken as upper case) or '*'; every other byte value breaks k-mers,
 *   the newline the reader puts behind each record included.  The letter that is hashed for a residue r:
 *     protein  r itself, upper case
 *     dayhoff  C -> a;  A G P S T -> b;  D E N Q -> c;  H K R -> d;  I L M V -> e;  F W Y -> f;  * -> *;  every other letter -> X
 *     hp       A F G I L M P V W Y -> h;  N C S T D E R H K Q -> p;  * -> *;  every other letter -> X
 * Protein input.  A k-mer is ksize (1 .. 64) consecutive residue bytes inside one source; its hash is the first word of
 *   MurmurHash3_x64_128 over its ksize encoded letters with `seed` (42); there is no canonical form; kept iff hash <= max_hash.
 * Translated input (KSP_SKETCH_TRANSLATE in flags).  The bytes are DNA with the rules above (ACGTacgt are bases, everything else
 *   breaks).  A window is 3 ksize consecutive bases inside one source, at EVERY position (all three frames); it yields two k-mers:
 *   the translation of its codons at offsets 0, 3, .. 3 ksize - 3, and the translation of the codons of its reverse complement.
 *   The standard genetic code, indexed by 16 b1 + 4 b2 + b3 with T, C, A, G = 0 .. 3:
 *     FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG
 *   Each translated k-mer is encoded and hashed as above, those with '*' like any other.  ksize is 1 .. 21 here (3 ksize <= 63
 *   bases fit the packed k-mer and the 64-byte halo); more is KSP_E_ARG naming the limit.  hp at sourmash's customary ksize 42
 *   therefore works on protein input only.
 * Sketch and counts.  A source's sketch is the ascending list of its distinct kept hashes.  The abundance of a hash is the number
 *   of (window, strand) pairs of the source that hash to it — for protein input the number of windows —, clamped at 2^32 - 1; a
 *   window whose two strands translate to the same k-mer counts twice.
 * ksp_sketch_text_hash: host only — the hash of the one k-mer that the `len` (1 .. 64) bytes of text spell for moltype 1 .. 3;
 *   *valid = 0 (and *hash = 0) when a byte is no residue.
 * ksp_sketch_cpu_mol / ksp_sketch_device_mol / ksp_sketch_host_mol: ksp_sketch_cpu / _device / _host with `moltype` and `flags`
 *   (KSP_SKETCH_TRANSLATE or 0) behind ksize, and the abundance output of the _abund calls, which may be NULL: one entry serves
 *   counted and plain.  moltype 0 without translate gives the DNA calls' results.  KSP_E_ARG: an unknown moltype, moltype 0 with
 *   translate, any other flag, ksize outside the limits above; otherwise the rules of the DNA calls.  stats->valid_kmers counts
 *   windows, stats->kept survivors (up to two per window when translating); ksp_sketch_host_mol's first capacity doubles when
 *   translating.  ksp_sketch_cpu_mol is the plain single-thread loop: the timing baseline and KSPIDER_SKETCH=host.
 * kspider_sketch with KSP_SKETCH_PROTEIN, _DAYHOFF or _HP in flags (more than one: KSP_E_ARG), and KSP_SKETCH_TRANSLATE beside one
 *   of them (alone: KSP_E_ARG): kSize is the RESIDUE k.  Without translate the input is protein, and a directory is searched for
 *   .faa .fa .fasta (each optionally .gz); with it the input is DNA in the files of the section above.  A record longer than a
 *   batch is cut with (window - 1) bytes of overlap, 3 kSize - 1 when translating; unions and added counts stay exact.  Every
 *   refusal happens before a device is chosen or a file is written.
 * The signature files: "molecule" is "protein", "dayhoff" or "hp"; "ksize" is 3 * kSize, and md5sum is taken over that decimal
 *   text followed by the mins — sourmash's stored form as far as it is known here (DESIGN.md 7r says what could not be checked).
 *   Downstream calls that take a kSize (kspider_pack, kspider_query, kspider_gather, kspider_pairwise_sigs, ksp_sig_read) therefore
 *   take 3 * kSize for these files.  The loaders select by "ksize" alone: do not mix DNA and protein signatures in a directory. */
#define KSP_MOL_DNA 0
#define KSP_MOL_PROTEIN 1
#define KSP_MOL_DAYHOFF 2
#define KSP_MOL_HP 3
#define KSP_SKETCH_PROTEIN 8ull
#define KSP_SKETCH_DAYHOFF 16ull
#define KSP_SKETCH_HP 32ull
#define KSP_SKETCH_TRANSLATE 64ull
int ksp_sketch_text_hash(const char* text, int len, int moltype, uint32_t seed, uint64_t* hash, int* valid);
int ksp_sketch_cpu_mol(const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, int moltype, uint64_t flags,
                       uint64_t max_hash, uint32_t seed, uint64_t* out_keys, uint32_t* out_abund, uint64_t capacity, uint64_t* out_offsets, uint64_t* needed);
int ksp_sketch_device_mol(int device, const uint8_t* d_seq, uint64_t n_bytes, const uint64_t* h_src_offsets, uint32_t n_sources, int ksize, int moltype,
                          uint64_t flags, uint64_t max_hash, uint32_t seed, uint64_t* d_out_keys, uint32_t* d_out_abund, uint64_t capacity,
                          uint64_t* h_out_offsets, ksp_sketch_stats* stats);
int ksp_sketch_host_mol(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize, int moltype,
                        uint64_t flags, uint64_t max_hash, uint32_t seed, uint64_t** out_keys, uint32_t** out_abund, uint64_t* out_offsets,
                        ksp_sketch_stats* stats);

/* ---- compare: counted sketches against each other — cosine, angular similarity, weighted containment (csrc/compare.hip,
 *      csrc/sketch_pack.cpp) ----
 * Sources are numbered as in query mode: database 0 .. n_db - 1, queries n_db .. n_db + n_q - 1.  Each side is its keys back to
 * back, host offsets, and an optional uint32_t abundance array parallel to the keys: abund[i] belongs to keys[i].  A NULL
 * abundance array means every abundance is 1, a flat sketch.  Runs are STRICTLY ASCENDING within a source and every abundance is
 * >= 1.  For a pair (s1 < s2) of the mode that shares at least one hash the row is a ksp_wedge: shared = the hashes in both,
 * dot = Σ over them of a_1(h) · a_2(h), mass_1 = Σ over them of a_1(h), mass_2 = Σ over them of a_2(h).  Per source the call also
 * returns sum[s] = Σ a and sumsq[s] = Σ a².  A source whose exact Σ a² is >= 2^64 is refused with KSP_E_LIMIT before any probe
 * runs; by Cauchy–Schwarz dot² <= sumsq_1 · sumsq_2, so every dot is then below 2^64, and a mass is at most its source's sum,
 * which is at most its Σ a²: the 64-bit adds cannot wrap and there is no saturation rule.  Everything on the device is an integer,
 * so the table is the same under every switch and schedule.
 * Modes: KSP_QUERY_CROSS and KSP_QUERY_CROSS_AND_SELF as in query mode, except that n_db = 0 is allowed with CROSS_AND_SELF — the
 *   pure all-pairs comparison of the queries; the database pointers may then be NULL.
 * ksp_compare_device: keys and abundances in DEVICE memory, offsets on the host.  The rows go to d_rows (device, room for
 *   `capacity`) in unspecified order; *n_rows = the rows found.  More than `capacity`: KSP_E_OVERFLOW, *n_rows is exact and nothing
 *   was written past `capacity`; d_rows NULL with capacity 0 is the size query.  h_sum / h_sumsq (host, n_db + n_q values each, may
 *   be NULL) are written once the totals are known, also by a call that overflows.  KSP_E_ARG, before a device is chosen: a NULL
 *   pointer (the abundances, h_sum, h_sumsq and stats may be NULL; the database's keys and offsets with n_db = 0), d_rows NULL
 *   with a capacity, n_q = 0, n_db = 0 with KSP_QUERY_CROSS, an unknown mode, offsets that do not start at 0 or decrease.
 *   KSP_E_ARG, found on the device before any probe, naming the side and the source: a run that is not strictly ascending, an
 *   abundance of 0.  Of several such sources the smallest in the common numbering is named, and a run out of order anywhere is
 *   reported before an abundance of 0 anywhere, also in a smaller source.  A run ascends inside its source only: it may end above
 *   or at the first key of the next.  A source may be empty: its totals are 0 and 0 and no row names it.  A side whose sources
 *   are all empty is accepted too (its key pointer is not NULL and is not read): all queries empty gives no row, the totals of every source and
 *   KSP_OK, and no table is built (stats.passes = 0).
 *   KSP_E_LIMIT: n_db + n_q > 2^32 - 2, Σ a² >= 2^64 (naming the side and the smallest such source), a query tile of 2^31
 *   entries or more, memory that does not fit the device's free memory (query mode's list, 4 bytes more per entry of the largest
 *   tile for the holders' abundances, 24 per source for the totals; the message says what was asked).  On the device: a check
 *   pass and a totals pass over both sides (Σ a² with a carry word), then per tile of at most KSP_COMPARE_TILE_MAX queries query
 *   mode's table, one pass that puts every query entry's abundance at its holder slot, and the probe, whose LDS counters are
 *   per query of the tile a u32 count and the u64 sums dot, mass_1, mass_2.  Read on every call: $KSP_COMPARE_TILE (1 ..
 *   KSP_COMPARE_TILE_MAX), $KSP_COMPARE_LONG_RUN (default KSP_QUERY_LONG_RUN), $KSP_COMPARE_LIST (1 .. KSP_COMPARE_LIST_MAX),
 *   $KSP_COMPARE_MAX_WORKGROUPS (caps the grids; tests).  The rows are the same under each.
 * ksp_compare_host: the same for HOST arrays: uploads, calls, retries once at the exact size, sorts the rows by (source_1,
 *   source_2) on the device and returns them in *rows (ksp_free).  sum / sumsq as above.  $KSP_COMPARE_FIRST_CAPACITY: the first
 *   call's capacity (tests: forces the retry).  A device that is not there: KSP_E_HIP, "ksp_compare_host: no such device".
 * ksp_compare_values: host only — the four derived values of a row, used by every writer.  n_i is the source's key count, kept for
 *   symmetry with the writers' per-source tables; no output uses it.  out[0] cosine = (double)dot / (sqrt((double)sumsq_1) ·
 *   sqrt((double)sumsq_2)), clamped to 1, and exactly 1 when dot² == sumsq_1 · sumsq_2 in 128-bit arithmetic (identical samples);
 *   out[1] angular = 1 − 2·acos(cosine)/π; out[2] weighted containment 1 = mass_1 / sum_1, the share of source 1's k-mer mass
 *   that lies on hashes source 2 also has; out[3] = mass_2 / sum_2.  KSP_E_ARG for a NULL pointer or a total of 0.
 * kspider_compare: `samples` is a directory of .sig / .sig.gz files (or whatever kspider_query takes; only signatures carry
 *   abundances, one without counts as all ones); `against` is NULL — every pair of samples — or a database, a directory or a
 *   pack file, flat or counted: then only database x sample rows.  Writes OUT.namesMap and OUT_kSpider_seqToKmersNo.tsv as
 *   kspider_query does (database ids first) and OUT_kSpider_compare.tsv: a header line, then per row source_1, source_2 (ids),
 *   shared_kmers, dot, mass_1, mass_2 in decimal and cosine, angular_similarity, weighted_containment_1, weighted_containment_2
 *   from ksp_compare_values printed "%.6g", sorted by (source_1, source_2).  flags KSP_COMPARE_MATRIX, without `against` only
 *   (else KSP_E_ARG): also OUT_kSpider_compare_matrix.csv — the names in the header line, then N rows of N angular similarities,
 *   1 on the diagonal, 0 where there is no row, symmetric, the TSV's text; KSP_E_LIMIT above KSP_COMPARE_MATRIX_MAX samples.
 *   Files go through .partial and a rename; a refused or failed call writes none.  Device = $KSPIDER_DEVICE (default 0).        */
#define KSP_COMPARE_TILE_MAX 512u     /* 14 KiB of counters per probe source in LDS: 28 bytes per query */
#define KSP_COMPARE_LIST_MAX 256u
#define KSP_COMPARE_MATRIX 1ull
#define KSP_COMPARE_MATRIX_MAX 16384u
typedef struct ksp_wedge {
    uint32_t source_1, source_2;
    uint64_t shared;   /* hashes in both                                   */
    uint64_t dot;      /* sum over shared hashes of a_1(h) * a_2(h)         */
    uint64_t mass_1;   /* sum over shared hashes of a_1(h)                  */
    uint64_t mass_2;   /* sum over shared hashes of a_2(h)                  */
} ksp_wedge;           /* 40 bytes */
typedef struct ksp_compare_stats {
    uint64_t n_db, n_q;
    uint64_t db_entries, q_entries;
    uint64_t table_keys, table_holders;   /* as in ksp_query_stats, summed over the tiles                     */
    uint64_t passes;
    uint64_t short_sources, long_sources;
    uint64_t list_overflows;
    uint64_t edges;            /* the rows found                                                       */
    uint64_t long_run;
    float ms_table, ms_probe;  /* HIP-event times, summed over the tiles                               */
    float ms_sort;             /* ksp_compare_host: the sort of the rows                               */
    float ms_totals;           /* the check pass and the totals pass                                   */
    float ms_holders;          /* the abundances to their holder slots, summed over the tiles          */
    uint32_t tile, list_capacity, reserved;
} ksp_compare_stats;   /* 128 bytes */
int ksp_compare_device(int device, const uint64_t* d_db_keys, const uint32_t* d_db_abund, const uint64_t* h_db_offsets, uint32_t n_db,
                       const uint64_t* d_q_keys, const uint32_t* d_q_abund, const uint64_t* h_q_offsets, uint32_t n_q, int mode,
                       ksp_wedge* d_rows, uint64_t capacity, uint64_t* n_rows, uint64_t* h_sum, uint64_t* h_sumsq, ksp_compare_stats* stats);
int ksp_compare_host(const uint64_t* db_keys, const uint32_t* db_abund, const uint64_t* db_offsets, uint32_t n_db, const uint64_t* q_keys,
                     const uint32_t* q_abund, const uint64_t* q_offsets, uint32_t n_q, int mode, int device, ksp_wedge** rows, uint64_t* n_rows,
                     uint64_t* sum, uint64_t* sumsq, ksp_compare_stats* stats);
int ksp_compare_values(const ksp_wedge* row, uint64_t n_1, uint64_t sum_1, uint64_t sumsq_1, uint64_t n_2, uint64_t sum_2, uint64_t sumsq_2,
                       double out[4]);
int kspider_compare(const char* samples, const char* against, int kSize, const char* out_prefix, int user_threads, uint64_t flags);

/* ---- classify: every read or contig against a sketch database (csrc/classify.hip, csrc/classify_kernels.hip.h,
 *      csrc/classify_cpu.cpp, csrc/classify_files.cpp) ----
 * The definition.  Records are DNA with the sketcher's rules unchanged: ACGTacgt are bases, every other byte breaks k-mers, a
 * k-mer is ksize (1 .. 64) bases inside one record, canonical form, Murmur's first word with `seed`, kept iff hash <= max_hash.
 * The references are n_refs STRICTLY ASCENDING runs of hashes back to back with host offsets (a counted signature is read as
 * flat).  For a record r: S(r) = the SET of its kept hashes; kept_windows(r) = the windows whose hash is kept (positions, so >=
 * |S(r)|); hits(r, q) = |S(r) ∩ ref_q|; matched(r) = |S(r) ∩ ⋃ ref_q|.  A row (r, q, hits) exists iff hits >= min_hits (>= 1);
 * rows are ordered by (r, q).  Per record, over its rows: n_refs_hit; best_ref = the reference of the largest hits, a tie going
 * to the smaller index (0xFFFFFFFF: no row); best_hits; second_hits = the largest hits among the record's OTHER rows (0: none).
 * Everything is an integer and nothing depends on scheduling.  This equals ksp_sketch_cpu per record followed by an intersection
 * with every reference.
 * Results of the one-shot calls and of _finish: *rows (ksp_free; never NULL after KSP_OK) with *n_rows, and six caller-owned
 *   arrays of n_records uint32_t: kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits.
 * ksp_classify_cpu: host only, single thread, over csrc/sketch_hash.h — the timing baseline and KSPIDER_CLASSIFY=host.
 * ksp_classify_host: the same on `device` for HOST arrays: one session, one batch (below).
 * The session, for a caller with batches: ksp_classify_open builds the table once; ksp_classify_add hashes one batch — n_segments
 *   segments of the byte stream (seg_offsets[n_segments + 1], ascending from 0 to n_bytes), segment s being a piece of record
 *   seg_records[s] (any id below 2^32 - 1; ids may repeat within and across batches).  A record cut across batches must have every
 *   window whole in exactly one piece (cut with ksize - 1 bytes of overlap); the same hash in two pieces counts once.
 *   ksp_classify_finish(n_records above every id added) returns the results and ends the session's work: after it only
 *   ksp_classify_close is allowed, which frees everything and may be called at any time (NULL is ignored).
 * On the device.  Table: query mode's collision-free table (csrc/query_table.hip.h) over ALL references, the tag being the
 *   reference index; reference hashes above max_hash are dropped first (they can never be hit).  Hash pass (k_classify_hash):
 *   the sketcher's tile frame — workgroups of 256 over tiles of KSP_SKETCH_TILE_BASES positions, $KSPIDER_SKETCH_MAX_WGS caps the
 *   grid — whose survivors are compacted by ballot into a list in LDS, drained in rounds by look-ups of four keys per lane; only
 *   hits leave the workgroup, as 64-bit words (record << 32) | table_index, one reservation per wave; the counter counts past
 *   the capacity and nothing is written at or past it.  A kept window adds 1 to kept_windows[record].  The hit words of all
 *   batches stay in one device buffer; a batch that does not fit first has the held words sorted and made unique (a compaction),
 *   then the buffer grown to the counted need, and its kernel run again (a retry).  $KSPIDER_CLASSIFY_FIRST_CAPACITY: the
 *   buffer's first capacity in words (tests).  Finish: radix sort and unique of the words (matched = words per record), every word
 *   expanded into (record << 32) | reference for each holder of its hash, sort, run lengths = hits, the cut at min_hits and the
 *   summary, all on the device.
 * KSP_E_ARG, before a device is chosen: a NULL pointer (stats may be NULL; ref_keys with no reference entry; seq with n_bytes 0),
 *   ksize outside 1 .. 64, n_records / n_segments = 0 (one-shot and _add), offsets that do not start at 0, decrease or do not end
 *   at n_bytes, reference offsets that do not start at 0 or decrease, a reference run that is not strictly ascending (naming the
 *   reference), min_hits = 0; _add: a record id of 2^32 - 1; _finish: n_records not above every id added; _add or _finish after
 *   _finish.  KSP_E_LIMIT: references that hold 2^31 entries or more (after the drop above), memory that does not fit the
 *   device's free memory (the message says how much was asked; nothing of that step has run, and a refused _add leaves the
 *   session as it was).  A device that is not there: KSP_E_HIP, "ksp_classify_open: no such device".
 * kspider_classify: the file driver.  input: one FASTA / FASTQ file or a directory (the sketcher's endings and glob order); EVERY
 *   record is a unit, its id its 1-based ordinal over the whole input; names may repeat.  db: a directory of .sig / .sig.gz files,
 *   or a pack file (kspider_pack); a group without a sketch of that kSize is never hit.  max_hash = ksp_sketch_max_hash(scaled),
 *   seed 42.  Batches of at most $KSPIDER_CLASSIFY_BATCH_MB (256; $KSPIDER_CLASSIFY_BATCH_BYTES: the same in bytes, at least 1024)
 *   through pinned staging, the next batch being read while the device works; a record longer than a batch is cut with ksize - 1
 *   bytes of overlap and the result does not depend on the batch size.  KSPIDER_CLASSIFY=host: the same driver over the host
 *   loop, no GPU.  Device = $KSPIDER_DEVICE (0).  KSPIDER_VERBOSE prints one line of the stats.  Writes, each through .partial and
 *   a rename, after everything was computed:
 *     OUT_kSpider_classify.tsv       record_id name length kept_windows matched n_refs best_ref best_hits second_hits — a header
 *                                    line, then one row per record in input order; best_ref is the reference's name, "-" for none;
 *                                    length = the bytes of the record's sequence
 *     OUT_kSpider_classify_hits.tsv  record_id name ref_id ref_name hits — a header line, then the rows by (record_id, ref_id);
 *                                    ref_id is the group's 1-based position in the database
 *   KSP_E_ARG: NULL or empty input / db / out_prefix, kSize outside 1 .. 64, scaled = 0, min_hits = 0, KSPIDER_CLASSIFY other than
 *   "host" / "device"; KSP_E_IO: no input file, a reader error, a database that cannot be read, a file that cannot be written. */
typedef struct ksp_classify_row {
    uint32_t record, reference, hits, reserved;
} ksp_classify_row;   /* 16 bytes */
typedef struct ksp_classify_stats {
    uint64_t bases;            /* base bytes of all batches (an overlap of a cut record counts in both pieces)          */
    uint64_t valid_kmers;      /* windows of ksize bases without a break byte, as in ksp_sketch_stats: the device counts
                                  one over a record boundary that no break byte marks (and drops it), the host loop does not */
    uint64_t kept_windows;     /* windows inside a record with hash <= max_hash: the sum of kept_windows[]               */
    uint64_t hit_words;        /* hit words appended by all batches (a retried batch counts once)                        */
    uint64_t hit_words_unique; /* distinct (record, table key) pairs: the sum of matched[]                               */
    uint64_t table_keys;       /* distinct reference hashes <= max_hash                                                  */
    uint64_t table_holders;    /* (hash, reference) pairs of the table                                                   */
    uint64_t batches;          /* ksp_classify_add calls that ran                                                        */
    uint64_t retries;          /* batches whose kernel ran a second time                                                 */
    uint64_t compactions;      /* sort + unique of the held words because a batch did not fit                            */
    uint64_t workgroups;       /* the largest grid of a hash pass                                                        */
    uint64_t rows;             /* rows returned                                                                          */
    float ms_table, ms_hash, ms_finish;   /* HIP-event times: the table; the hash passes, summed; the finish (0 on the host) */
    uint32_t reserved;
} ksp_classify_stats;   /* 112 bytes */
typedef struct ksp_classify ksp_classify;
int ksp_classify_cpu(const uint8_t* seq, uint64_t n_bytes, const uint64_t* rec_offsets, uint32_t n_records, int ksize, uint64_t max_hash,
                     uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs, uint32_t min_hits,
                     ksp_classify_row** rows, uint64_t* n_rows, uint32_t* kept_windows, uint32_t* matched, uint32_t* n_refs_hit,
                     uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits, ksp_classify_stats* stats);
int ksp_classify_host(int device, const uint8_t* seq, uint64_t n_bytes, const uint64_t* rec_offsets, uint32_t n_records, int ksize,
                      uint64_t max_hash, uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs,
                      uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows, uint32_t* kept_windows, uint32_t* matched,
                      uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits, ksp_classify_stats* stats);
int ksp_classify_open(int device, int ksize, uint64_t max_hash, uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets,
                      uint32_t n_refs, ksp_classify** out);
int ksp_classify_add(ksp_classify* c, const uint8_t* seq, uint64_t n_bytes, const uint64_t* seg_offsets, const uint32_t* seg_records,
                     uint32_t n_segments);
int ksp_classify_finish(ksp_classify* c, uint32_t n_records, uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows,
                        uint32_t* kept_windows, uint32_t* matched, uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits,
                        uint32_t* second_hits, ksp_classify_stats* stats);
void ksp_classify_close(ksp_classify* c);
int kspider_classify(const char* input, int kSize, uint64_t scaled, const char* db, const char* out_prefix, int user_threads,
                     uint32_t min_hits);

/* ---- host-only diagnostics (no GPU needed) -------------------------------------------
 * ksp_index_info: parse the three index files and report what the reader detected:
 * out[0] colours, out[1] groups, out[2] colour-count entries, out[3] sum of sources over
 * colours, out[4] phmap Group::kWidth (16/8), out[5] 1 if a growth_left trailer is present.
 * ksp_format_float: text of a float as `std::ostream << float` prints it
 * (src/pairwise.cpp:266-273); buf must hold 32 bytes; returns the length.             */
int ksp_index_info(const char* index_prefix, uint64_t out[6]);
int ksp_format_float(float value, char* buf);
/* ksp_ani_value: the ANI of a row whose containment floats are min_c / max_c (see above) for k-mer size ksize.
 * via_table 0: the text definition ("%.6g" -> strtod -> libm pow); 1: the device's code path on the host (exact
 * 6-digit decimal of each float, then the table the device reads).  KSP_E_ARG on a NaN.  ksp_ani_values: n rows at
 * once (a NaN row gets NaN and the call returns KSP_E_ARG).  ksp_format_ani: text of a double as Python's repr()
 * prints it (the ANI column's format); buf must hold 32 bytes; returns the length.                                */
int ksp_ani_value(float min_c, float max_c, int ksize, int via_table, double* out);
int ksp_ani_values(const float* min_c, const float* max_c, uint64_t n, int ksize, int via_table, double* out);
int ksp_format_ani(double value, char* buf);

#ifdef __cplusplus
}
#endif
#endif /* KSPIDER_AMD_H */
