// Internal declarations shared by the engine (engine.hip), the multi-device job (multi.hip), the consumers of the
// join's edges and the host-side reference surface (pairwise_host.cpp).  Not part of the C ABI.
#ifndef KSPIDER_ENGINE_INTERNAL_H
#define KSPIDER_ENGINE_INTERNAL_H
#include <cstdint>
#include <functional>
#include <string>

#include "../../include/kspider_amd.h"

#include <vector>

namespace ksp {
void set_error(const std::string& s);
// GPUs of a drop-in call: $KSPIDER_DEVICES ("0,1,2,..."; a device may appear twice) or the one of $KSPIDER_DEVICE (0)
std::vector<int> devices_from_env();

// ---- clustering straight from the join's edges (cluster.hip) ----
// the smallest float the reference's threshold test lets through (mode 1: only NaN rows pass)
void cc_critical(double cutoff, float* vcrit, int* mode);
// connected components of the kept edges among d_edges (device memory of the CURRENT device): h_label[v] = smallest
// node of v's component; d_cnt[v] = k-mer count of node v; col 3 / 4 / 5 = min / avg / max containment, 6 = the average
// ANI of `pairwise --estimate-ani` for k-mer size ksize (ani.h; KSP_E_ARG if an edge has a NaN containment)
int cc_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double cutoff,
                       uint32_t* h_label, uint64_t* n_kept, int ksize = 0);
// The edges of cc_rounds_on_device, one of three forms, all in device memory of the CURRENT device: the join's records cut by
// cc_edge_kept (ed, cnt, col 3 / 4 / 5, vcrit / mode of cc_critical; strict: a record naming a node >= n_nodes and a self pair
// are skipped before anything is read through them), the records whose bit in keep[] is set (ed, keep), or pairs (a, b).
struct CcRounds {
    const ksp_edge* ed = nullptr;
    const unsigned long long* keep = nullptr;
    const uint32_t *a = nullptr, *b = nullptr, *cnt = nullptr;
    int col = 0, mode = 0;
    float vcrit = 0;
    bool strict = false;
};
// the rounds of cc_edges_on_device alone: d_parent (n_nodes words, set by cc_init_on_device) ends as the labels and stays on the
// device; d_changed: 4 words of scratch; *n_kept (may be NULL; the cut records only): the records the cut keeps
int cc_init_on_device(uint32_t n_nodes, uint32_t* d_parent);
int cc_rounds_on_device(const CcRounds& edges, uint32_t n_nodes, uint64_t n_edges, uint32_t* d_parent, uint32_t* d_changed, uint64_t* n_kept);
void read_names_map(const std::string& prefix, std::vector<std::string>& name_of);
void write_cluster_file(const std::string& prefix, double threshold, const std::vector<uint32_t>& label,
                        const std::vector<std::string>& name_of);
// the same lines to a file of the caller's name (through .partial and a rename)
void write_cluster_file_as(const std::string& out_path, const std::vector<uint32_t>& label, const std::vector<std::string>& name_of);
// ---- neighbour counts straight from the join's edges (repr.hip; apps/repr_sketches.cpp) ----
// the text test of the reference on one float: "%.6g" text -> strtof -> as double -> > threshold
bool repr_text_passes(float v, double threshold);
// the smallest non-negative float that passes it (*none_pass = 1: not even +inf passes, nothing is counted)
void repr_critical(double threshold, float* vcrit, int* none_pass);
// neighbour counts of the edges among d_edges (device memory of the CURRENT device) whose column col passes the text test,
// and their ranking by (count descending, node ascending); see ksp_edges_degrees / ksp_edges_repr.  h_degree (n_nodes
// entries) or h_node / h_count / n_ranked may be NULL: that half is not computed.
int repr_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double threshold,
                         uint32_t* h_degree, uint32_t* h_node, uint32_t* h_count, uint32_t* n_ranked);
// "id: count\n" per ranked node (id = ids[node]) to out_path through out_path.partial and a rename, or to stdout ("")
void write_repr_file(const std::string& out_path, const std::vector<uint32_t>& ids, const uint32_t* node, const uint32_t* count, uint64_t n_ranked);
// ---- the containment cut on the join's edges, before they are gathered, sorted and copied (cut.hip) ----
// what the count pass leaves for the scatter pass (device memory of the device it ran on; release() frees it)
struct CutPass {
    uint64_t n_chunks = 0;
    uint64_t* d_off = nullptr;                 // n_chunks + 1 exclusive offsets: the last is the total
    unsigned long long* d_ballots = nullptr;   // one kept bit per record, or NULL: the scatter evaluates the predicate again
    float vcrit = 0;                           // cc_critical of the cut-off
    int mode = 0;
    void release();
};
// count + scan over d_edges (device memory of the CURRENT device): *n_kept = records whose column col is kept by cc_edge_kept
int cut_count_on_device(const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double cutoff, CutPass& pass, uint64_t* n_kept);
// the kept records into d_out (room for *n_kept of them), in their input order; nothing behind them is written
int cut_scatter_on_device(const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, const CutPass& pass, ksp_edge* d_out);
// ---- the cut-off ladder: components at a list of cut-offs from one pass over the join's edges (sweep.hip) ----
// ksp_components_edges_sweep on the CURRENT device: h_labels = n_cutoffs x n_nodes in the caller's order, h_kept may be NULL
int sweep_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, const double* cutoffs,
                          uint32_t n_cutoffs, uint32_t* h_labels, uint64_t* h_kept);
// one cluster file per distinct cut-off and PREFIX_kSpider_cluster_sweep_<dist>.tsv (cluster.hip); labels: n_cutoffs rows of
// name_of.size() node labels in the caller's order, kept[i]: the rows cut-off i keeps
void write_sweep_outputs(const std::string& prefix, const std::string& dist, const double* cutoffs, uint32_t n_cutoffs, const uint32_t* labels,
                         const uint64_t* kept, const std::vector<std::string>& name_of);
// ---- the single-linkage tree: a maximum spanning forest of the join's edges (tree.hip) ----
// ksp_edges_forest on the CURRENT device; preload: a load and compare before every atomic (what ships); *rounds may be NULL
int tree_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, uint32_t* h_index,
                         uint32_t* n_forest, bool preload = true, uint32_t* rounds = nullptr);
// one row of a tree file: node indices (id - 1), the weight that orders the rows (the value kspider_cluster tests, float(text) x
// 100), the value itself (the newick heights) and its text
struct TreeRow {
    uint32_t a, b;
    double weight, value;
    std::string text;
};
// PREFIX_kSpider_tree_<dist>.tsv (and .newick) from the rows of a spanning forest, in any order
void write_tree_files(const std::string& prefix, const std::string& dist, std::vector<TreeRow>& rows, const std::vector<std::string>& name_of, bool newick);
// a kept row names its nodes by id - 1: the ids must be rows of .namesMap (throws)
void check_row_nodes(long long a, long long b, uint64_t n_names);
// ---- dereplication: greedy representatives and their members from the join's edges (derep.hip) ----
// (repr.hip) the counting kernel and the key kernel on the caller's device buffers: d_degree[n_nodes] and the key of EVERY node
int degree_keys_on_device(uint32_t n_nodes, const ksp_edge* d_edges, const uint32_t* d_a, const uint32_t* d_b, uint64_t n_edges, const uint32_t* d_cnt,
                          int col, float vcrit, uint32_t* d_degree, uint64_t* d_keys);
// what the last selection on this thread did: the rounds the host dispatched, the rounds of the tail kernel (0: it did not run)
// and the live pairs when it took over; kept: records that became oriented pairs
struct DerepTrace {
    uint64_t dispatched = 0, tail = 0, live_at_tail = 0, kept = 0;
};
// ksp_edges_dereplicate on the CURRENT device; h_via / h_rank / h_degree may be NULL; *trace may be NULL
int derep_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double threshold,
                          uint32_t* h_rep, uint32_t* h_via, uint32_t* h_rank, uint32_t* h_degree, uint32_t* n_reps, DerepTrace* trace = nullptr);
// one source of a dereplication file: its representative (itself: a representative), the text of the assigning record's value
struct DerepRow {
    uint32_t rep = 0, degree = 0, rank = 0;
    std::string text;
};
// out_path (through out_path.partial and a rename): "source\trepresentative\t<dist>\tneighbours\trank", one row per name
void write_derep_file(const std::string& out_path, const std::string& dist, const std::vector<DerepRow>& rows, const std::vector<std::string>& name_of);
// ---- top-k neighbours: each source's best hits from the join's edges (topk.hip) ----
// what the last selection on this thread did: the nodes selected by the wave, workgroup and stream kernels (all 0 with
// KSP_TOPK_SELECT=library) and the refills of the stream kernel, summed over its nodes
struct TopkTrace {
    uint64_t wave = 0, workgroup = 0, stream = 0, refills = 0;
};
// ksp_edges_topk on the CURRENT device (1 <= k <= KSP_TOPK_MAX_K, h_index n_nodes x k, h_count n_nodes); *trace may be NULL
int topk_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, uint32_t k, uint32_t* h_index,
                         uint32_t* h_count, TopkTrace* trace = nullptr);
// out_path (through out_path.partial and a rename): "source\thit\tneighbour\t<dist>", one row per hit, the sources in the order of
// the names; count[v]: the hits of name v, neighbour / text: the other end and the value text of every hit, flat in that order
void write_topk_file(const std::string& out_path, const std::string& dist, const std::vector<std::string>& name_of, const std::vector<uint32_t>& count,
                     const std::vector<uint32_t>& neighbour, const std::vector<std::string>& text);
// ---- the cluster report: density, medoid and coverage of every cluster from the join's edges (report.hip) ----
// what the last report on this thread did: the kept records, the chunks whose kept records carried one label (their cluster sums
// left the workgroup as one set of atomics), the sets of cluster atomics and the sets of source_1-side node atomics issued
struct ReportTrace {
    uint64_t kept = 0, single_label_chunks = 0, cluster_sets = 0, node_sets = 0;
};
// ksp_edges_cluster_report on the CURRENT device (h_cluster / h_member: n_nodes rows); *trace may be NULL
int report_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, double cutoff,
                           ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member, ReportTrace* trace = nullptr);
// PREFIX_kSpider_cluster_report_<dist>_<P>%.tsv and PREFIX_kSpider_cluster_members_<dist>_<P>%.tsv, P = py_float_repr(threshold),
// both through .partial and a rename: the clusters in order of their root (the lines of write_cluster_file), the members in the
// order of the names.  via_text[v]: the value text of member v's `via` record ("" without one).
void write_report_files(const std::string& prefix, const std::string& dist, double threshold, const std::vector<ksp_cluster_row>& cluster,
                        const std::vector<ksp_member_row>& member, const std::vector<std::string>& via_text, const std::vector<std::string>& name_of);
// ---- the average-linkage tree (UPGMA) of the join's edges, exact, on the sparse edge list (upgma.hip) ----
// what the last tree on this thread did: the records taking part, the pairs after the first fold, the device rounds, the merges
// made on the device, the live pairs handed to the host finish, its merges, and the longest run a fold inside a round summed
struct UpgmaTrace {
    uint64_t taking_part = 0, first_pairs = 0, rounds = 0, device_merges = 0, handed_over = 0, host_merges = 0, longest_run = 0;
};
// ksp_edges_upgma on the CURRENT device (h_rows: room for n_nodes - 1 rows); *trace may be NULL
int upgma_edges_on_device(uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, int col, ksp_upgma_row* h_rows,
                          uint32_t* n_rows, UpgmaTrace* trace = nullptr);
// PREFIX_kSpider_upgma_<dist>.tsv (and .newick) from the rows in merge order (node indices of name_of), through .partial and a
// rename; on a failure every file this call created is removed again
void write_upgma_files(const std::string& prefix, const std::string& dist, const std::vector<ksp_upgma_row>& rows, const std::vector<std::string>& name_of,
                       bool newick);
// ---- the rows of the pairwise TSV as text, made on the device from the join's edges (tsv.hip) ----
// takes the next piece of the text (it lives until the call returns); a code other than KSP_OK, with its text in
// ksp_last_error(), ends the pass
typedef std::function<int(const char*, uint64_t)> TsvSink;
// ksp_edges_tsv on the CURRENT device: *n_bytes = the bytes of the text; sink NULL: nothing else (the size query), otherwise the
// text goes to *sink in order, in pieces of at most $KSP_TSV_PIECE bytes, unless capacity < *n_bytes (KSP_E_OVERFLOW, nothing
// is handed out).  d_ids NULL: a source's id is its index.  ms_kernels (may be NULL): the device time of the passes.
int tsv_edges_on_device(const char* who, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_cnt, const uint32_t* d_ids,
                        uint64_t capacity, const TsvSink* sink, uint64_t* n_bytes, float* ms_kernels = nullptr);
// ---- what a job wants from its edges besides the edges themselves: one kind per job ----
// kCut: only the edges that pass a containment cut are wanted, so every device cuts its own directly after its join and only the
// kept ones are gathered, sorted and copied.  The other kinds are taken from the sorted edges on the first device, while they
// are in HBM: the components (cc_edges_on_device), the ranking (repr_edges_on_device), the components at every cut-off of a
// ladder (sweep_edges_on_device), the maximum spanning forest (tree_edges_on_device), the dereplicated set (derep_edges_on_device),
// the k best hits of every source (topk_edges_on_device), the report of every cluster (report_edges_on_device), the average-linkage
// tree (upgma_edges_on_device).
struct AfterJoin {
    enum Kind { kNone, kCluster, kRepr, kCut, kSweep, kTree, kDerep, kTopk, kReport, kUpgma };
    Kind kind = kNone;
    const uint32_t* kmer_counts = nullptr;   // per (dense) source index
    int col = 0;                             // 3 / 4 / 5; kCluster: also 6 = ANI
    int ksize = 0;                           // kCluster: k-mer size of the ANI column (col 6)
    double cutoff = 0;                       // kCluster, kCut, kReport
    double threshold = 0.20;                 // kRepr, kDerep
    const double* cutoffs = nullptr;         // kSweep
    uint32_t n_cutoffs = 0;                  //   1 .. KSP_SWEEP_MAX_CUTOFFS
    uint32_t k = 0;                          // kTopk: 1 .. KSP_TOPK_MAX_K
    // out
    std::vector<uint32_t> labels;            // kCluster: per source index, the smallest index of its component; kSweep: n_cutoffs such rows
    uint64_t n_kept = 0;                     // kCluster: edges that passed the cut
    std::vector<uint64_t> kept;              // kSweep: edges that passed each cut-off
    std::vector<uint32_t> node, count;       // kRepr: the sources with a neighbour, (count descending, index ascending), and their counts
    uint64_t n_found = 0;                    // kCut: edges before the cut, summed over the devices
    std::vector<uint32_t> index;             // kTree: the forest's records as indices into the returned (sorted) edges, in merge order
    std::vector<uint32_t> rep, via, degree;  // kDerep: per source index its representative, the assigning record (0xFFFFFFFF: none), its neighbours;
    DerepTrace derep;                        //   the ranks are in `node` (rank[v]); what the selection did
    TopkTrace topk;                          // kTopk: per source index its hits in `index` (n_sources x k records of the returned edges) and
                                             //   their number in `count`; what the selection did
    std::vector<ksp_cluster_row> cluster_rows;   // kReport: the clusters in order of their root (source indices), and per source index
    std::vector<ksp_member_row> member_rows;     //   its row; `via` is a record of the returned edges; what the passes did
    ReportTrace report;
    std::vector<ksp_upgma_row> upgma_rows;   // kUpgma: the merges in merge order (source indices); what the rounds did
    UpgmaTrace upgma;
    // The rows' text, wanted besides whatever `kind` asks for (KSPIDER_TSV=device): the text pass runs on the first device over
    // the gathered, sorted edges, after the consumer.  ids: the id of every source index (n_sources entries).  text_sink takes
    // the pieces in file order.  With kNone and kCut nobody reads the records afterwards, so they are not copied to the host:
    // the job returns no edges (an empty array) with their number.
    bool want_text = false;
    const uint32_t* ids = nullptr;
    TsvSink text_sink;
    uint64_t text_bytes = 0;                 // out: the bytes handed to text_sink
    bool edges_skipped = false;              // out: the records stayed on the device
};
int pairwise_postings_multi_cc(const uint64_t* key_off, const uint32_t* sources, const uint32_t* key_weights, uint32_t n_keys,
                               uint32_t n_sources, const int* devices, int n_devices, ksp_edge** out_edges, uint64_t* n_edges,
                               ksp_stats* stats, AfterJoin* after);
// ---- sketching (sketch_cpu.cpp, sketcher.hip, fastx_reader.cpp, sketch_files.cpp) ----
// what ksp_sketch_cpu / _device / _host refuse with KSP_E_ARG: a NULL pointer, ksize outside 1 .. 64, no source, offsets that do
// not start at 0, decrease or do not end at n_bytes
int check_sketch_args(const char* who, const void* seq, uint64_t n_bytes, const uint64_t* src_offsets, uint32_t n_sources, int ksize);
// what the _mol calls refuse with KSP_E_ARG before that: an unknown moltype, a flag other than KSP_SKETCH_TRANSLATE,
// translate with KSP_MOL_DNA, ksize outside 1 .. 21 with translate (the message names the limit) and outside 1 .. 64 without
int check_sketch_mol(const char* who, int ksize, int moltype, uint64_t flags);
// page-locked host memory for the batches of the file driver (sketcher.hip; NULL when it cannot be had)
void* pinned_alloc(size_t bytes);
void pinned_free(void* p);
// a file, gzip or plain, whole (sketch_loaders.cpp; throws std::runtime_error naming the file)
std::string read_maybe_gz(const std::string& path);
// One FASTA / FASTQ file (fastx_reader.cpp; throws std::runtime_error naming the file and the line): seq = every record's bases
// as they stand in the file followed by one '\n', rec_off[records + 1] their bounds, names = every header's first word.
struct FastxFile {
    std::string seq;
    std::vector<uint64_t> rec_off;
    std::vector<std::string> names;
    bool fastq = false;
};
void read_fastx(const std::string& path, FastxFile& out);
// ---- classify (classify_cpu.cpp, classify.hip, classify_files.cpp) ----
// what the classify calls refuse with KSP_E_ARG about their references: NULL offsets, NULL keys with an entry, ksize outside
// 1 .. 64, offsets that do not start at 0 or decrease, a run that is not strictly ascending (naming the reference)
int check_classify_refs(const char* who, int ksize, const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs);
// ... and about a batch: NULL pointers, no segment, offsets that do not start at 0, decrease or do not end at n_bytes, a record
// id of 2^32 - 1 (seg_records NULL: segment s is record s)
int check_classify_batch(const char* who, const void* seq, uint64_t n_bytes, const uint64_t* seg_offsets, const uint32_t* seg_records, uint32_t n_segments);
// ... and about the results: a NULL pointer, min_hits = 0
int check_classify_out(const char* who, uint32_t min_hits, const void* rows, const void* n_rows, const void* kept_windows, const void* matched, const void* n_refs_hit,
                       const void* best_ref, const void* best_hits, const void* second_hits);
// The host loop's session: the form of ksp_classify_open / _add / _finish on the host, single thread, for ksp_classify_cpu and
// the file driver's host mode.  Arguments are checked by the caller; the methods return a KSP_* code and never throw.
class ClassifyCpu {
    struct State;
    State* s_ = nullptr;

public:
    ClassifyCpu() = default;
    ClassifyCpu(const ClassifyCpu&) = delete;
    ClassifyCpu& operator=(const ClassifyCpu&) = delete;
    ~ClassifyCpu();
    int open(const char* who, int ksize, uint64_t max_hash, uint32_t seed, const uint64_t* ref_keys, const uint64_t* ref_offsets, uint32_t n_refs);
    int add(const char* who, const uint8_t* seq, const uint64_t* seg_offsets, const uint32_t* seg_records, uint32_t n_segments);
    int finish(const char* who, uint32_t n_records, uint32_t min_hits, ksp_classify_row** rows, uint64_t* n_rows, uint32_t* kept_windows, uint32_t* matched,
               uint32_t* n_refs_hit, uint32_t* best_ref, uint32_t* best_hits, uint32_t* second_hits, ksp_classify_stats* stats);
};
}

extern "C" {
/* test/diagnostic hook: distinct-key offsets of the block lists (nb + 1 values). */
int ksp_engine_block_key_counts(const ksp_engine* e, uint32_t* h_blk_off);
int ksp_engine_source_order(const ksp_engine* e, uint32_t* h_newidx);   // (diagnostics) engine index of every source
/* (tools/cut_times.py) HIP-event times of `reps` cuts of one list: which 0 = hand-written, predicate evaluated in both passes,
 * 1 = hand-written with kept ballots, 2 = rocprim::select with the same predicate. */
int ksp_debug_cut_times(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, double cutoff,
                        ksp_edge* d_out, int which, int reps, float* ms, uint64_t* n_kept);
/* (tests) the two kernels of the cut-off ladder without the components: d_level[n_edges] (device) = the level of every record,
 * cut-offs counted in order of strictness; band l = [h_band_off[l - 1], h_band_off[l]) of d_a / d_b (device, room for the edges
 * of level >= 1), l = 1 .. n_cutoffs: the endpoints of the edges of level l, in any order. */
int ksp_debug_sweep_bands(int device, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, const double* cutoffs,
                          uint32_t n_cutoffs, uint8_t* d_level, uint64_t* h_band_off, uint32_t* d_a, uint32_t* d_b);
/* (tools/sweep_times.py) HIP-event times of `reps` runs of: which 0 = ksp_components_edges_sweep, 1 = one ksp_components_edges per cut-off. */
int ksp_debug_sweep_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                          const double* cutoffs, uint32_t n_cutoffs, int which, int reps, float* ms, uint32_t* h_labels);
/* (tools/tree_times.py) HIP-event times of `reps` runs of ksp_edges_forest's device part: which 0 = as shipped, 1 = no load before the atomics. */
int ksp_debug_tree_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                         int which, int reps, float* ms, uint32_t* h_index, uint32_t* n_forest, uint32_t* rounds);
/* (tests) what the last ksp_edges_dereplicate / kspider_dereplicate of this thread did: out[0] the rounds the host dispatched, out[1]
 * the rounds of the tail kernel (0: it did not run), out[2] the live pairs when it took over, out[3] the records that became oriented pairs. */
int ksp_debug_derep_rounds(uint64_t out[4]);
/* (tests) what the last ksp_edges_topk / ksp_topk_ranked / kspider_topk of this thread did: out[0] / out[1] / out[2] the nodes selected by
 * the wave, workgroup and stream kernels (0 with KSP_TOPK_SELECT=library), out[3] the refills of the stream kernel over all its nodes. */
int ksp_debug_topk_classes(uint64_t out[4]);
/* (tests) what the last ksp_edges_cluster_report / ksp_cluster_report_valued of this thread did: out[0] the kept records, out[1] the
 * chunks that took the single-label path, out[2] the sets of cluster atomics issued, out[3] the sets of source_1-side node atomics. */
int ksp_debug_report_counts(uint64_t out[4]);
/* (tests) what the last ksp_edges_upgma / ksp_upgma_valued / kspider_upgma of this thread did: out[0] the pairs after the first fold, out[1]
 * the device rounds, out[2] the merges made on the device, out[3] the live pairs at the hand-over, out[4] the merges made by the host
 * finish, out[5] the longest run a fold inside a round summed (0: no round folded a run above 1). */
int ksp_debug_upgma_counts(uint64_t out[6]);
/* (tools/upgma_times.py) HIP-event times of `reps` whole runs of ksp_edges_upgma over the same records (allocations, copies and the
 * host finish included): ms[reps]; counts: ksp_debug_upgma_counts of the last run. */
int ksp_debug_upgma_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col, int reps,
                          float* ms, ksp_upgma_row* h_rows, uint32_t* n_rows, uint64_t counts[6]);
/* (tools/report_times.py) HIP-event times of `reps` runs over the same records.  ms holds 5 x reps values: ms[5r] the whole device part
 * of ksp_edges_cluster_report (allocations and the copies to the host included), ms[5r + 1 .. 5r + 3] its accumulate, medoid and links
 * passes alone, ms[5r + 4] the whole of ksp_components_edges on the same records, for comparison: the labels are what both pay. */
int ksp_debug_report_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                           double cutoff, int reps, float* ms, ksp_cluster_row* h_cluster, uint32_t* n_clusters, ksp_member_row* h_member);
/* (tools/topk_times.py) HIP-event times of `reps` runs of ksp_edges_topk's device part: which 0 = the hand-written select kernels,
 * 1 = rocprim::segmented_radix_sort_keys and a gather (KSP_TOPK_SELECT=library). */
int ksp_debug_topk_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, int dist_col,
                         uint32_t k, int which, int reps, float* ms, uint32_t* h_index, uint32_t* h_count);
/* (tools/query_times.py) HIP-event times of `reps` device-to-device copies of `bytes` bytes: the copy rate of the session, the
 * yardstick of the query probe's floor (8 bytes per database hash). */
int ksp_debug_copy_times(int device, uint64_t bytes, int reps, float* ms);
/* (tests) the device's "%.6g" (tsv_text.h) on n host floats: h_text[16 * i ...] holds the h_len[i] bytes of value i's text.  KSP_E_ARG,
 * with nothing written, when a value is outside the domain: 0, +inf and the positive floats in [2^-40, 2^40). */
int ksp_debug_format_floats(int device, const float* h_values, uint64_t n, char* h_text /* n x 16 */, uint32_t* h_len);
/* (tests) the yardstick in the same layout: ksp_format_float (the host's snprintf) on every value; KSP_E_ARG for a text above 16 bytes. */
int ksp_debug_format_floats_host(const float* h_values, uint64_t n, char* h_text /* n x 16 */, uint32_t* h_len);
/* (tools/tsv_times.py) valid seeded inputs of the timing, made on the device: ids index + 1, counts of 10^3 .. 10^6, n_edges records with
 * source_1 ascending and below source_2 and a shared count of 1 .. the smaller count.  All three arrays are device memory. */
int ksp_debug_tsv_records(int device, uint32_t n_nodes, uint64_t n_edges, uint64_t seed, ksp_edge* d_edges, uint32_t* d_kmer_counts, uint32_t* d_ids);
/* (tools/tsv_times.py) `reps` runs of one way from the records in device memory to the rows' text in host memory, without a file:
 * which 0 = the device's text kernels and the copy of the text to pinned host memory, 1 = the copy of the records to pinned host
 * memory and the host writer's formatting (index_io.cpp format_rows) with `threads` host threads.  ms holds 2 x reps values:
 * ms[2r] the wall time of run r, ms[2r + 1] which 0: the kernels' own time by HIP events, which 1: the time of the copy. */
int ksp_debug_tsv_times(int device, uint32_t n_nodes, const ksp_edge* d_edges, uint64_t n_edges, const uint32_t* d_kmer_counts, const uint32_t* d_ids,
                        int which, int reps, int threads, float* ms);
}
#endif
