"""ctypes binding of the C ABI in ``include/kspider_amd.h``.

Everything here goes through ``libkspider_amd.so`` (hand-written HIP for gfx950).
There is no CPU fallback: if the library is missing or no MI355X is visible the
calls raise.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KSPIDER_AMD_LIB") or os.path.join(_HERE, "lib", "libkspider_amd.so")   # (override: A/B timing of two builds)

EDGE_DTYPE = np.dtype([("source_1", "<u4"), ("source_2", "<u4"), ("shared", "<u8")])

KSP_OK, KSP_E_ARG, KSP_E_HIP, KSP_E_IO, KSP_E_OVERFLOW, KSP_E_LIMIT = range(6)

#: records per chunk of the containment cut's two passes (kCutChunkEdges in csrc/cut.hip = KSP_CUT_CHUNK_EDGES in the header)
CUT_CHUNK_EDGES = 2048

#: records per chunk of the cut-off ladder's two passes and its longest ladder (KSP_SWEEP_CHUNK_EDGES / KSP_SWEEP_MAX_CUTOFFS in the header)
SWEEP_CHUNK_EDGES = 2048
SWEEP_MAX_CUTOFFS = 255

#: records per chunk of the edge passes of the single-linkage tree (KSP_TREE_CHUNK_EDGES in the header)
TREE_CHUNK_EDGES = 2048

#: entries per chunk of the dereplication's edge passes, and the live pairs at which one workgroup finishes the rounds
#: (KSP_DEREP_CHUNK_EDGES / KSP_DEREP_TAIL_PAIRS in the header)
DEREP_CHUNK_EDGES = 2048
DEREP_TAIL_PAIRS = 65536

#: top-k neighbours (KSP_TOPK_* in the header): records per chunk of the edge passes; the entries up to which a node is selected
#: by one wave, and by one workgroup in LDS (anything larger is streamed); the largest k
TOPK_CHUNK_EDGES = 2048
TOPK_WAVE_ENTRIES = 64
TOPK_LDS_ENTRIES = 4096
TOPK_MAX_K = 1024

#: records per chunk of the cluster report's edge passes (KSP_REPORT_CHUNK_EDGES in the header)
REPORT_CHUNK_EDGES = 2048

#: ksp_cluster_row / ksp_member_row of the header (48 and 24 bytes)
CLUSTER_ROW_DTYPE = np.dtype([("root", "<u4"), ("size", "<u4"), ("edges", "<u8"), ("nan_edges", "<u8"), ("sum_q", "<u8"), ("min", "<f4"), ("max", "<f4"),
                              ("medoid", "<u4"), ("covered", "<u4")])
MEMBER_ROW_DTYPE = np.dtype([("label", "<u4"), ("degree", "<u4"), ("strength", "<u8"), ("via", "<u4"), ("reserved", "<u4")])

#: the average-linkage tree (KSP_UPGMA_* in the header): entries per chunk of its passes; the live pairs at or below which the host
#: finishes (measured: DESIGN.md 7m); ksp_upgma_row (24 bytes)
UPGMA_CHUNK_EDGES = 2048
UPGMA_TAIL_PAIRS = 1024
UPGMA_ROW_DTYPE = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("sum_q", "<u8"), ("size_lo", "<u4"), ("size_hi", "<u4")])

#: the device's row text (KSP_TSV_* in the header): rows per chunk of the text passes, the shortest and the longest row in bytes
TSV_CHUNK_ROWS = 256
TSV_ROW_MIN = 12
TSV_ROW_MAX = 79

#: query mode (include/kspider_amd.h KSP_QUERY_*): the modes, the largest tile and touched list, the default short/long switch
QUERY_CROSS, QUERY_CROSS_AND_SELF = 0, 1
QUERY_TILE_MAX = 2048
QUERY_LIST_MAX = 512
QUERY_LONG_RUN = 2048
QUERY_DIR_BITS_MAX = 24

#: gather (include/kspider_amd.h KSP_GATHER_*): rounds per batch, the default switches, the first candidate buffer, the row record
GATHER_BATCH = 16
GATHER_LONG_SEG = 1024
GATHER_TAIL_CANDS = 256
GATHER_TAIL_CANDS_MAX = 1 << 20
GATHER_FIRST_CANDS = 4096
GATHER_ROW_DTYPE = np.dtype([("query", np.uint32), ("rank", np.uint32), ("source", np.uint32), ("overlap", np.uint32), ("unique", np.uint32),
                             ("remaining", np.uint32)])
#: ksp_gather_wrow: the weighted row, 64 bytes (the 128-bit sum of squares as two words)
GATHER_WROW_DTYPE = np.dtype([("query", np.uint32), ("rank", np.uint32), ("source", np.uint32), ("overlap", np.uint32), ("unique", np.uint32),
                              ("remaining", np.uint32), ("w_unique", np.uint64), ("w_found", np.uint64), ("sq_lo", np.uint64), ("sq_hi", np.uint64),
                              ("median2", np.uint64)])

#: compare (include/kspider_amd.h KSP_COMPARE_*): the largest tile and touched list, the matrix flag and its limit, ksp_wedge (40 bytes)
COMPARE_TILE_MAX = 512
COMPARE_LIST_MAX = 256
COMPARE_MATRIX = 1
COMPARE_MATRIX_MAX = 16384
WEDGE_DTYPE = np.dtype([("source_1", np.uint32), ("source_2", np.uint32), ("shared", np.uint64), ("dot", np.uint64), ("mass_1", np.uint64), ("mass_2", np.uint64)])

#: the sketcher (csrc/sketcher.hip): positions per tile of the hash pass; the flags of kspider_sketch
SKETCH_TILE_BASES = 4096
SKETCH_PER_RECORD, SKETCH_SEED, SKETCH_ABUND = 1, 2, 4
#: protein sketches: the molecule types of the _mol calls, their flags of kspider_sketch, six-frame translation
MOL_DNA, MOL_PROTEIN, MOL_DAYHOFF, MOL_HP = 0, 1, 2, 3
SKETCH_PROTEIN, SKETCH_DAYHOFF, SKETCH_HP, SKETCH_TRANSLATE = 8, 16, 32, 64
_MOLTYPES = {"dna": MOL_DNA, "protein": MOL_PROTEIN, "dayhoff": MOL_DAYHOFF, "hp": MOL_HP}

#: classify (csrc/classify.hip): a row of the hits table; "no reference" in best_ref
CLASSIFY_ROW_DTYPE = np.dtype([("record", np.uint32), ("reference", np.uint32), ("hits", np.uint32), ("reserved", np.uint32)])
CLASSIFY_NO_REF = 0xFFFFFFFF

#: ksp_engine_lists_path / Engine.lists_path
LISTS_NONE, LISTS_KEYED, LISTS_COMPACTED, LISTS_SORTED, LISTS_FUSED = 0, 1, 2, 3, 4

#: every symbol include/kspider_amd.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "ksp_last_error", "ksp_device_count", "ksp_engine_create", "ksp_engine_destroy",
    "ksp_engine_build_blocks", "ksp_engine_num_tiles", "ksp_engine_tile_pairs", "ksp_engine_join",
    "ksp_engine_join_launch", "ksp_engine_join_wait", "ksp_engine_join_to_host", "ksp_engine_step_launch",
    "ksp_engine_get_stats", "ksp_device_malloc", "ksp_device_free", "ksp_memcpy_h2d", "ksp_memcpy_d2h",
    "ksp_pairwise_host", "ksp_free", "kspider_pairwise", "ksp_index_info", "ksp_format_float",
    "kspider_pairwise_sigs", "kspider_pairwise_bins",
    "ksp_engine_build_slice", "ksp_engine_slice_sizes", "ksp_engine_slice_export", "ksp_engine_assemble",
    "ksp_engine_edge_bound", "ksp_engine_slice_labels", "ksp_engine_slice_finish",
    "ksp_engine_slice_bounds", "ksp_engine_slice_set_bounds", "ksp_engine_balanced_cuts",
    "ksp_engine_build_postings", "ksp_engine_build_postings_slice", "ksp_pairwise_postings_host",
    "ksp_engine_set_profiling", "ksp_engine_phase_times", "ksp_engine_lists_path",
    "ksp_pairwise_host_multi", "ksp_pairwise_postings_host_multi",
    "kspider_cluster", "ksp_components", "ksp_components_edges", "kspider_pairwise_and_cluster",
    "kspider_estimate_ani", "kspider_pairwise_ani", "kspider_pairwise_ani_and_cluster", "ksp_edges_ani",
    "ksp_components_edges_ani", "ksp_ani_value", "ksp_ani_values", "ksp_format_ani",
    "kspider_export", "ksp_single_linkage_rows", "ksp_single_linkage_prim", "ksp_row_distances",
    "ksp_csv_float",
    "ksp_edges_degrees", "ksp_edges_repr", "ksp_repr_critical", "kspider_repr_sketches", "kspider_pairwise_and_repr",
    "ksp_edges_cut", "ksp_pairwise_host_cut", "kspider_pairwise_cut",
    "ksp_components_edges_sweep", "ksp_components_sweep", "kspider_cluster_sweep", "kspider_pairwise_and_cluster_sweep",
    "ksp_edges_forest", "ksp_forest_ranked", "kspider_tree", "kspider_pairwise_and_tree", "kspider_cluster_from_tree",
    "ksp_edges_dereplicate", "kspider_dereplicate", "kspider_pairwise_and_dereplicate",
    "ksp_edges_topk", "ksp_topk_ranked", "kspider_topk", "kspider_pairwise_and_topk",
    "ksp_edges_cluster_report", "ksp_cluster_report_valued", "kspider_cluster_report", "kspider_pairwise_and_cluster_report",
    "ksp_edges_upgma", "ksp_upgma_valued", "ksp_upgma_before", "kspider_upgma", "kspider_pairwise_and_upgma", "kspider_cluster_from_upgma",
    "ksp_edges_tsv",
    "ksp_query_device", "ksp_query_host", "ksp_query_directory", "kspider_pack", "ksp_pack_info", "ksp_pack_load", "kspider_query",
    "ksp_gather_device", "ksp_gather_host", "kspider_gather",
    "ksp_gather_abund_device", "ksp_gather_abund_host", "kspider_gather_abund",
    "ksp_compare_device", "ksp_compare_host", "ksp_compare_values", "kspider_compare",
    "ksp_sketch_cpu_abund", "ksp_sketch_device_abund", "ksp_sketch_host_abund", "ksp_sig_read",
    "ksp_sketch_max_hash", "ksp_murmur64", "ksp_sketch_kmer_hash", "ksp_sketch_cpu", "ksp_sketch_device", "ksp_sketch_host",
    "ksp_fastx_info", "ksp_fastx_load", "kspider_sketch",
    "ksp_sketch_text_hash", "ksp_sketch_cpu_mol", "ksp_sketch_device_mol", "ksp_sketch_host_mol",
    "ksp_classify_cpu", "ksp_classify_host", "ksp_classify_open", "ksp_classify_add", "ksp_classify_finish", "ksp_classify_close", "kspider_classify",
]


class Stats(ctypes.Structure):
    _fields_ = [
        ("n_sources", ctypes.c_uint64), ("n_entries", ctypes.c_uint64), ("n_blocks", ctypes.c_uint64),
        ("n_block_keys", ctypes.c_uint64), ("n_tiles", ctypes.c_uint64), ("last_tiles", ctypes.c_uint64),
        ("last_pairs", ctypes.c_uint64), ("last_stream_bytes", ctypes.c_uint64), ("last_edges", ctypes.c_uint64),
        ("ms_build", ctypes.c_float), ("ms_join", ctypes.c_float), ("weighted", ctypes.c_int),
        ("key_bits", ctypes.c_int), ("n_active_tiles", ctypes.c_uint64), ("last_active_tiles", ctypes.c_uint64),
        ("sort_entries", ctypes.c_uint64), ("ms_sort", ctypes.c_float), ("sort_bits", ctypes.c_int),
        ("partition_kind", ctypes.c_int), ("partition_fallback", ctypes.c_int),
        ("n_match_records", ctypes.c_uint64), ("n_join_workgroups", ctypes.c_uint64),
        ("n_kept_entries", ctypes.c_uint64), ("n_kept_keys", ctypes.c_uint64),
        ("stage1_kind", ctypes.c_int), ("big_buckets", ctypes.c_int),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class QueryStats(ctypes.Structure):
    """ksp_query_stats (include/kspider_amd.h)."""
    _fields_ = [
        ("n_db", ctypes.c_uint64), ("n_q", ctypes.c_uint64), ("db_entries", ctypes.c_uint64), ("q_entries", ctypes.c_uint64),
        ("table_keys", ctypes.c_uint64), ("table_holders", ctypes.c_uint64), ("passes", ctypes.c_uint64),
        ("short_sources", ctypes.c_uint64), ("long_sources", ctypes.c_uint64), ("list_overflows", ctypes.c_uint64),
        ("edges", ctypes.c_uint64), ("long_run", ctypes.c_uint64),
        ("ms_table", ctypes.c_float), ("ms_probe", ctypes.c_float), ("ms_sort", ctypes.c_float),
        ("tile", ctypes.c_uint32), ("list_capacity", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class CompareStats(ctypes.Structure):
    """ksp_compare_stats (include/kspider_amd.h): 128 bytes."""
    _fields_ = [
        ("n_db", ctypes.c_uint64), ("n_q", ctypes.c_uint64), ("db_entries", ctypes.c_uint64), ("q_entries", ctypes.c_uint64),
        ("table_keys", ctypes.c_uint64), ("table_holders", ctypes.c_uint64), ("passes", ctypes.c_uint64),
        ("short_sources", ctypes.c_uint64), ("long_sources", ctypes.c_uint64), ("list_overflows", ctypes.c_uint64),
        ("edges", ctypes.c_uint64), ("long_run", ctypes.c_uint64),
        ("ms_table", ctypes.c_float), ("ms_probe", ctypes.c_float), ("ms_sort", ctypes.c_float), ("ms_totals", ctypes.c_float), ("ms_holders", ctypes.c_float),
        ("tile", ctypes.c_uint32), ("list_capacity", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class Wedge(ctypes.Structure):
    """ksp_wedge (include/kspider_amd.h): 40 bytes."""
    _fields_ = [("source_1", ctypes.c_uint32), ("source_2", ctypes.c_uint32), ("shared", ctypes.c_uint64), ("dot", ctypes.c_uint64), ("mass_1", ctypes.c_uint64),
                ("mass_2", ctypes.c_uint64)]


class GatherStats(ctypes.Structure):
    """ksp_gather_stats (include/kspider_amd.h)."""
    _fields_ = [
        ("n_db", ctypes.c_uint64), ("n_q", ctypes.c_uint64), ("db_entries", ctypes.c_uint64), ("q_entries", ctypes.c_uint64),
        ("table_keys", ctypes.c_uint64), ("table_holders", ctypes.c_uint64), ("passes", ctypes.c_uint64),
        ("candidates", ctypes.c_uint64), ("dropped", ctypes.c_uint64), ("fell_below", ctypes.c_uint64), ("slots", ctypes.c_uint64),
        ("rounds", ctypes.c_uint64), ("batches", ctypes.c_uint64), ("tail_rounds", ctypes.c_uint64), ("live_at_tail", ctypes.c_uint64),
        ("rows", ctypes.c_uint64), ("long_seg", ctypes.c_uint64), ("tail_cands", ctypes.c_uint64),
        ("ms_table", ctypes.c_float), ("ms_candidates", ctypes.c_float), ("ms_fill", ctypes.c_float), ("ms_rounds", ctypes.c_float),
        ("tile", ctypes.c_uint32), ("min_hashes", ctypes.c_uint32), ("max_matches", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class GatherWRow(ctypes.Structure):
    """ksp_gather_wrow (include/kspider_amd.h): 64 bytes."""
    _fields_ = [("query", ctypes.c_uint32), ("rank", ctypes.c_uint32), ("source", ctypes.c_uint32), ("overlap", ctypes.c_uint32), ("unique", ctypes.c_uint32),
                ("remaining", ctypes.c_uint32), ("w_unique", ctypes.c_uint64), ("w_found", ctypes.c_uint64), ("sq_lo", ctypes.c_uint64), ("sq_hi", ctypes.c_uint64),
                ("median2", ctypes.c_uint64)]


class SketchStats(ctypes.Structure):
    """ksp_sketch_stats (include/kspider_amd.h)."""
    _fields_ = [
        ("bases", ctypes.c_uint64), ("valid_kmers", ctypes.c_uint64), ("kept", ctypes.c_uint64), ("distinct_out", ctypes.c_uint64),
        ("needed", ctypes.c_uint64), ("workgroups", ctypes.c_uint64), ("retries", ctypes.c_uint64),
        ("ms_upload", ctypes.c_float), ("ms_hash", ctypes.c_float), ("ms_select", ctypes.c_float), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class ClassifyStats(ctypes.Structure):
    """ksp_classify_stats (include/kspider_amd.h): 112 bytes."""
    _fields_ = [
        ("bases", ctypes.c_uint64), ("valid_kmers", ctypes.c_uint64), ("kept_windows", ctypes.c_uint64), ("hit_words", ctypes.c_uint64),
        ("hit_words_unique", ctypes.c_uint64), ("table_keys", ctypes.c_uint64), ("table_holders", ctypes.c_uint64), ("batches", ctypes.c_uint64),
        ("retries", ctypes.c_uint64), ("compactions", ctypes.c_uint64), ("workgroups", ctypes.c_uint64), ("rows", ctypes.c_uint64),
        ("ms_table", ctypes.c_float), ("ms_hash", ctypes.c_float), ("ms_finish", ctypes.c_float), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class KspError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"kspider_amd error {code}: {msg}")
        self.code = code


class PrevJoinError(KspError):
    """Engine.step_launch: the join of the previous step failed (``code`` is its status), but this call's step went
    ahead all the same — ``step`` is the (t0, t1, bound, launched, prev_count) that step_launch would have returned."""

    def __init__(self, code, msg, step):
        super().__init__(code, msg)
        self.step = step


_lib = None


def lib():
    """Load libkspider_amd.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(the HIP extension is mandatory, there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        L.ksp_last_error.restype = ctypes.c_char_p
        L.ksp_engine_num_tiles.restype = ctypes.c_uint64
        L.ksp_engine_num_tiles.argtypes = [ctypes.c_void_p]
        L.ksp_engine_tile_pairs.restype = ctypes.c_uint64
        L.ksp_engine_edge_bound.restype = ctypes.c_uint64
        L.ksp_engine_balanced_cuts.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_engine_edge_bound.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
        L.ksp_engine_tile_pairs.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
        L.ksp_engine_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.ksp_engine_destroy.argtypes = [ctypes.c_void_p]
        L.ksp_engine_destroy.restype = None
        L.ksp_engine_build_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        L.ksp_engine_join.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p,
                                      ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.ksp_engine_get_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(Stats)]
        L.ksp_engine_join_launch.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.ksp_engine_join_wait.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_engine_build_slice.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_void_p]
        L.ksp_engine_slice_sizes.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_engine_slice_labels.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_engine_slice_bounds.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_engine_slice_set_bounds.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_engine_slice_finish.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_engine_slice_export.argtypes = [ctypes.c_void_p] + [ctypes.c_void_p] * 7
        L.ksp_engine_assemble.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.ksp_device_malloc.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.POINTER(ctypes.c_void_p)]
        L.ksp_device_free.argtypes = [ctypes.c_void_p]
        L.ksp_memcpy_h2d.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.ksp_memcpy_d2h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.ksp_pairwise_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Stats)]
        L.ksp_free.argtypes = [ctypes.c_void_p]
        L.ksp_pairwise_host_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Stats)]
        L.ksp_pairwise_postings_host_multi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                                       ctypes.c_uint32, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64),
                                                       ctypes.POINTER(Stats)]
        L.ksp_engine_build_postings.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        L.ksp_engine_build_postings_slice.argtypes = L.ksp_engine_build_postings.argtypes
        L.ksp_pairwise_postings_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                                 ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Stats)]
        L.ksp_free.restype = None
        L.ksp_engine_set_profiling.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.ksp_engine_lists_path.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        L.ksp_engine_phase_times.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p),
                                             ctypes.POINTER(ctypes.c_float), ctypes.c_int]
        L.kspider_cluster.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double]
        L.ksp_components.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.c_void_p]
        L.kspider_pairwise.argtypes = [ctypes.c_char_p, ctypes.c_int]
        L.ksp_index_info.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_format_float.argtypes = [ctypes.c_float, ctypes.c_char_p]
        L.kspider_pairwise_sigs.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.kspider_pairwise_bins.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        L.kspider_estimate_ani.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int64]
        L.kspider_pairwise_ani.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int64]
        L.kspider_pairwise_ani_and_cluster.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double]
        L.ksp_edges_ani.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
        L.ksp_components_edges_ani.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                               ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
        L.ksp_ani_value.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double)]
        L.ksp_ani_values.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.ksp_format_ani.argtypes = [ctypes.c_double, ctypes.c_char_p]
        L.kspider_export.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]
        L.ksp_single_linkage_rows.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_single_linkage_prim.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_row_distances.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_csv_float.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double)]
        L.ksp_edges_degrees.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                        ctypes.c_double, ctypes.c_void_p]
        L.ksp_edges_repr.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                     ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.ksp_repr_critical.argtypes = [ctypes.c_double, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)]
        L.kspider_repr_sketches.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double, ctypes.c_char_p]
        L.kspider_pairwise_and_repr.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double, ctypes.c_char_p]
        L.ksp_edges_cut.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                    ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_pairwise_host_cut.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_double, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(Stats)]
        L.kspider_pairwise_cut.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double]
        L.ksp_components_edges_sweep.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_components_sweep.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                           ctypes.c_uint32, ctypes.c_void_p]
        L.kspider_cluster_sweep.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32]
        L.kspider_pairwise_and_cluster_sweep.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_uint32]
        L.ksp_debug_sweep_bands.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_edges_forest.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.ksp_forest_ranked.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                        ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
        L.kspider_tree.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        L.kspider_pairwise_and_tree.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.kspider_cluster_from_tree.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double]
        L.ksp_edges_dereplicate.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_uint32)]
        L.kspider_dereplicate.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double, ctypes.c_char_p]
        L.kspider_pairwise_and_dereplicate.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double, ctypes.c_char_p]
        L.ksp_debug_derep_rounds.argtypes = [ctypes.c_void_p]
        L.ksp_edges_topk.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_topk_ranked.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32,
                                      ctypes.c_void_p, ctypes.c_void_p]
        L.kspider_topk.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
        L.kspider_pairwise_and_topk.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
        L.ksp_debug_topk_classes.argtypes = [ctypes.c_void_p]
        L.ksp_edges_cluster_report.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_cluster_report_valued.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.kspider_cluster_report.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double]
        L.kspider_pairwise_and_cluster_report.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double]
        L.ksp_debug_report_counts.argtypes = [ctypes.c_void_p]
        L.ksp_debug_report_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_edges_upgma.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_upgma_valued.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_upgma_before.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int)]
        L.kspider_upgma.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]
        L.kspider_pairwise_and_upgma.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.kspider_cluster_from_upgma.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_double]
        L.ksp_debug_upgma_counts.argtypes = [ctypes.c_void_p]
        L.ksp_debug_upgma_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_edges_tsv.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_debug_format_floats.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_debug_format_floats_host.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_debug_tsv_records.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_debug_tsv_times.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                          ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.ksp_query_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_query_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_query_directory.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        L.kspider_pack.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
        L.ksp_pack_info.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
        L.ksp_pack_load.argtypes = [ctypes.c_char_p] + [ctypes.c_void_p] * 6
        L.kspider_query.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]
        L.ksp_gather_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_gather_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                      ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.kspider_gather.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        L.ksp_gather_abund_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_gather_abund_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.kspider_gather_abund.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]
        L.ksp_compare_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_compare_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.ksp_compare_values.argtypes = [ctypes.POINTER(Wedge)] + [ctypes.c_uint64] * 6 + [ctypes.POINTER(ctypes.c_double)]
        L.kspider_compare.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64]
        L.ksp_sketch_cpu_abund.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_sketch_device_abund.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64,
                                              ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        L.ksp_sketch_host_abund.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        L.ksp_sig_read.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                   ctypes.POINTER(ctypes.c_int)]
        L.ksp_sketch_max_hash.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_murmur64.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
        L.ksp_sketch_kmer_hash.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        L.ksp_sketch_cpu.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32,
                                     ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_sketch_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64,
                                        ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        L.ksp_sketch_host.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64,
                                      ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        L.ksp_fastx_info.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
        L.ksp_fastx_load.argtypes = [ctypes.c_char_p] + [ctypes.c_void_p] * 4
        L.kspider_sketch.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64]
        L.ksp_sketch_text_hash.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int)]
        L.ksp_sketch_cpu_mol.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
        L.ksp_sketch_device_mol.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                            ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        L.ksp_sketch_host_mol.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_uint64,
                                          ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(SketchStats)]
        _classify_out = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64)] + [ctypes.c_void_p] * 6 + [ctypes.POINTER(ClassifyStats)]
        _classify_in = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.c_uint32, ctypes.c_uint32]
        L.ksp_classify_cpu.argtypes = _classify_in + _classify_out
        L.ksp_classify_host.argtypes = [ctypes.c_int] + _classify_in + _classify_out
        L.ksp_classify_open.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                        ctypes.POINTER(ctypes.c_void_p)]
        L.ksp_classify_add.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        L.ksp_classify_finish.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32] + _classify_out
        L.ksp_classify_close.argtypes = [ctypes.c_void_p]
        L.ksp_classify_close.restype = None
        L.kspider_classify.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint32]
        _lib = L
    return _lib


def _check(rc):
    if rc != KSP_OK:
        raise KspError(rc, lib().ksp_last_error().decode(errors="replace"))


def device_count() -> int:
    n = ctypes.c_int(0)
    _check(lib().ksp_device_count(ctypes.byref(n)))
    return n.value


def pairwise_host(keys: np.ndarray, offsets: np.ndarray, weights: np.ndarray | None = None, device: int = 0,
                  devices: list | None = None):
    """Host sketches -> (edges sorted by (source_1, source_2), stats).  IDs are dense 0..N-1.
    `devices`: shard the job over several GPUs (ksp_pairwise_host_multi; a device may be named twice)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    n = offsets.size - 1
    out = ctypes.c_void_p()
    ne = ctypes.c_uint64(0)
    st = Stats()
    devs = (ctypes.c_int * len(devices))(*devices) if devices else (ctypes.c_int * 1)(device)
    _check(lib().ksp_pairwise_host_multi(keys.ctypes.data, w.ctypes.data if w is not None else None, offsets.ctypes.data,
                                         n, devs, len(devs), ctypes.byref(out), ctypes.byref(ne), ctypes.byref(st)))
    edges = _take(out, ne.value, EDGE_DTYPE)
    return edges, st.as_dict()


def pairwise(index_prefix: str, user_threads: int = 1) -> None:
    """kSpider::pairwise(index_prefix, user_threads) through the C ABI (reference: kSpider.hpp:11)."""
    _check(lib().kspider_pairwise(os.fsencode(index_prefix), int(user_threads)))


def pairwise_sigs(sigs_dir: str, kSize: int, out_prefix: str | None = None, user_threads: int = 1) -> None:
    """sourmash signatures -> pairwise TSVs (= sourmash_sigs_indexing(sigs_dir, kSize) + pairwise())."""
    _check(lib().kspider_pairwise_sigs(os.fsencode(sigs_dir), int(kSize),
                                       os.fsencode(out_prefix) if out_prefix else None, int(user_threads)))


def pairwise_bins(bins_dir: str, out_prefix: str | None = None, user_threads: int = 1) -> None:
    """phmap flat_hash_set<uint64> sketch dumps (*.bin) -> pairwise TSVs."""
    _check(lib().kspider_pairwise_bins(os.fsencode(bins_dir), os.fsencode(out_prefix) if out_prefix else None,
                                       int(user_threads)))


def pairwise_postings_host(key_off: np.ndarray, sources: np.ndarray, key_weights: np.ndarray | None, n_sources: int,
                           device: int = 0, devices: list | None = None):
    """Inverted index (key k held by sources[key_off[k]:key_off[k+1]], weight key_weights[k] or 1) ->
    (edges sorted by (source_1, source_2), stats).  What the drop-in path feeds the engine."""
    key_off = np.ascontiguousarray(key_off, dtype=np.uint64)
    sources = np.ascontiguousarray(sources, dtype=np.uint32)
    kw = None if key_weights is None else np.ascontiguousarray(key_weights, dtype=np.uint32)
    out = ctypes.c_void_p()
    n = ctypes.c_uint64(0)
    st = Stats()
    devs = (ctypes.c_int * len(devices))(*devices) if devices else (ctypes.c_int * 1)(device)
    _check(lib().ksp_pairwise_postings_host_multi(key_off.ctypes.data, sources.ctypes.data,
                                                  kw.ctypes.data if kw is not None else None, key_off.size - 1, n_sources,
                                                  devs, len(devs), ctypes.byref(out), ctypes.byref(n), ctypes.byref(st)))
    edges = _take(out, n.value, EDGE_DTYPE)
    return edges, st.as_dict()


def cluster(index_prefix: str, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """`kSpider cluster -i PREFIX -d DIST -c CUTOFF` (ks_clustering.py:150-163); components on the GPU."""
    _check(lib().kspider_cluster(os.fsencode(index_prefix), dist_type.encode(), float(cutoff)))


def pairwise_and_cluster(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """`kSpider pairwise` + `kSpider cluster` in one device pass: both TSVs as the two calls would write them, the
    components taken from the edges while they are in HBM (the pairwise TSV is never read back)."""
    L = lib()
    L.kspider_pairwise_and_cluster.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_double]
    _check(L.kspider_pairwise_and_cluster(os.fsencode(index_prefix), int(user_threads), dist_type.encode(), float(cutoff)))


def components_edges(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int, cutoff: float,
                     device: int = 0) -> np.ndarray:
    """Components over ksp_edge records in DEVICE memory: an edge counts when its containment column passes the
    reference's cut (include/kspider_amd.h); label[v] = smallest source index of v's component."""
    L = lib()
    L.ksp_components_edges.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_double, ctypes.c_void_p]
    out = np.empty(max(1, n_nodes), dtype=np.uint32)
    _check(L.ksp_components_edges(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, dist_col, float(cutoff),
                                  out.ctypes.data))
    return out[:n_nodes]


def edges_degrees(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 4, threshold: float = 0.20,
                  device: int = 0) -> np.ndarray:
    """Neighbour counts over ksp_edge records in DEVICE memory (apps/repr_sketches.cpp): degree[v] = records naming v whose
    containment column passes the reference's text test against `threshold` (include/kspider_amd.h)."""
    out = np.zeros(max(1, n_nodes), dtype=np.uint32)
    _check(lib().ksp_edges_degrees(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), float(threshold),
                                   out.ctypes.data))
    return out[:n_nodes]


def edges_repr(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 4, threshold: float = 0.20,
               device: int = 0) -> tuple:
    """(nodes, counts): the nodes with a neighbour, ranked on the device by (count descending, node ascending)."""
    node = np.zeros(max(1, n_nodes), dtype=np.uint32)
    count = np.zeros(max(1, n_nodes), dtype=np.uint32)
    n = ctypes.c_uint32(0)
    _check(lib().ksp_edges_repr(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), float(threshold),
                                node.ctypes.data, count.ctypes.data, ctypes.byref(n)))
    return node[:n.value].copy(), count[:n.value].copy()


def repr_critical(threshold: float = 0.20) -> tuple:
    """(vcrit, none_pass): the smallest non-negative float whose 6-digit text, read back with strtof, is > threshold, as a
    numpy float32; none_pass: not even +inf passes.  Host only."""
    v = ctypes.c_float(0)
    none = ctypes.c_int(0)
    _check(lib().ksp_repr_critical(float(threshold), ctypes.byref(v), ctypes.byref(none)))
    return np.float32(v.value), bool(none.value)


def repr_sketches(pairwise_tsv: str, dist_type: str | None = None, threshold: float = 0.20, out_path: str | None = None) -> None:
    """The reference's `repr_sketches TSV` over an existing pairwise TSV: "id: count" lines, count descending then id
    ascending, to out_path (None: stdout).  The device counts and ranks."""
    _check(lib().kspider_repr_sketches(os.fsencode(pairwise_tsv), dist_type.encode() if dist_type is not None else None, float(threshold),
                                       os.fsencode(out_path) if out_path else None))


def pairwise_and_repr(index_prefix: str, user_threads: int = 1, dist_type: str | None = None, threshold: float = 0.20,
                      out_path: str | None = None) -> None:
    """`kSpider pairwise` + `repr_sketches` in one device pass: both TSVs as kspider_pairwise writes them, plus the ranking
    (None: PREFIX_kSpider_repr_sketches.txt), counted from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_repr(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                           float(threshold), os.fsencode(out_path) if out_path else None))


def edges_cut(d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, d_out_ptr: int, dist_col: int = 5, cutoff: float = 0.0,
              device: int = 0) -> int:
    """The containment cut over ksp_edge records in DEVICE memory (include/kspider_amd.h): the records `kSpider cluster`
    would keep for this column and cut-off go to d_out in their input order; returns how many.  d_out[kept:] is not written."""
    n = ctypes.c_uint64(0)
    _check(lib().ksp_edges_cut(device, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), float(cutoff),
                               d_out_ptr or None, ctypes.byref(n)))
    return int(n.value)


def pairwise_host_cut(keys: np.ndarray, offsets: np.ndarray, weights: np.ndarray | None = None, kmer_counts: np.ndarray | None = None,
                      dist_col: int = 5, cutoff: float = 0.0, devices=(0,)):
    """pairwise_host with the containment cut made on every device directly after its join: (kept edges sorted by
    (source_1, source_2), edges found before the cut, stats).  kmer_counts None: the run lengths."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    kc = None if kmer_counts is None else np.ascontiguousarray(kmer_counts, dtype=np.uint32)
    if kc is not None and kc.size != offsets.size - 1:
        raise ValueError("kmer_counts needs one entry per source")
    out = ctypes.c_void_p()
    ne = ctypes.c_uint64(0)
    nf = ctypes.c_uint64(0)
    st = Stats()
    devs = (ctypes.c_int * len(devices))(*devices)
    _check(lib().ksp_pairwise_host_cut(keys.ctypes.data, w.ctypes.data if w is not None else None, offsets.ctypes.data, offsets.size - 1,
                                       kc.ctypes.data if kc is not None else None, int(dist_col), float(cutoff), devs, len(devs),
                                       ctypes.byref(out), ctypes.byref(ne), ctypes.byref(nf), ctypes.byref(st)))
    edges = _take(out, ne.value, EDGE_DTYPE)
    return edges, int(nf.value), st.as_dict()


def pairwise_cut(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """`kSpider pairwise` with a minimum containment: the pairwise TSV holds only the rows `kSpider cluster -d DIST -c CUTOFF`
    would keep, cut on the device before the sort, the copy and the text; seqToKmersNo is not affected."""
    _check(lib().kspider_pairwise_cut(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                      float(cutoff)))


def _cutoff_array(cutoffs):
    """(array or None, count): None stands for a NULL list, as the C ABI sees it."""
    if cutoffs is None:
        return None, 0
    c = np.ascontiguousarray(np.asarray(cutoffs, dtype=np.float64).reshape(-1))
    return c, c.size


def cluster_sweep(index_prefix: str, dist_type: str = "max_cont", cutoffs=(0.0,)) -> None:
    """`kSpider cluster -i PREFIX -d DIST -c C` at every cut-off of the list from one reading of the pairwise TSV and one
    device pass: a cluster file per distinct cut-off as `cluster` writes it, plus PREFIX_kSpider_cluster_sweep_<DIST>.tsv."""
    c, k = _cutoff_array(cutoffs)
    _check(lib().kspider_cluster_sweep(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None,
                                       c.ctypes.data if c is not None and k else None, k))


def pairwise_and_cluster_sweep(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", cutoffs=(0.0,)) -> None:
    """`pairwise_and_cluster` at every cut-off of the list: the pairwise TSV of `pairwise`, the clusters of every cut-off from
    one pass over the edges while they are in HBM; the files of `cluster_sweep`."""
    c, k = _cutoff_array(cutoffs)
    _check(lib().kspider_pairwise_and_cluster_sweep(os.fsencode(index_prefix), int(user_threads),
                                                    dist_type.encode() if dist_type is not None else None,
                                                    c.ctypes.data if c is not None and k else None, k))


def components_edges_sweep(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int, cutoffs,
                           device: int = 0) -> tuple:
    """(labels[K, n_nodes], kept[K]): `components_edges` at every cut-off of the list over ksp_edge records in DEVICE memory,
    from one classification of the records and one continued components computation (include/kspider_amd.h)."""
    c, k = _cutoff_array(cutoffs)
    kept = np.zeros(max(1, k), dtype=np.uint64)
    flat = np.empty(max(1, k * n_nodes), dtype=np.uint32)
    _check(lib().ksp_components_edges_sweep(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col),
                                            c.ctypes.data if c is not None and k else None, k, flat.ctypes.data, kept.ctypes.data))
    labels = flat[:k * n_nodes].reshape(k, n_nodes)
    return labels, kept[:k]


def components_sweep(n_nodes: int, a: np.ndarray, b: np.ndarray, level: np.ndarray, n_levels: int, device: int = 0) -> np.ndarray:
    """labels[n_levels, n_nodes] of host edges that are already classified (level[e] in 0..n_levels): row r = the components
    of the edges with level > r, each labelled by its smallest node."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    level = np.ascontiguousarray(level, dtype=np.uint8)
    if not (a.size == b.size == level.size):
        raise ValueError("a, b and level need one entry per edge")
    k = max(0, int(n_levels))
    flat = np.empty(max(1, k * n_nodes), dtype=np.uint32)
    _check(lib().ksp_components_sweep(device, n_nodes, a.ctypes.data, b.ctypes.data, level.ctypes.data, a.size, int(n_levels), flat.ctypes.data))
    return flat[:k * n_nodes].reshape(k, n_nodes)


def sweep_bands(d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int, cutoffs, d_level_ptr: int, d_a_ptr: int, d_b_ptr: int,
                device: int = 0) -> np.ndarray:
    """(tests) The two kernels of the cut-off ladder without the components (ksp_debug_sweep_bands, csrc/engine_internal.h): the
    level byte of every record to d_level, the endpoints of the edges of level l to band l of d_a / d_b; returns the K + 1 band
    offsets (band l = [off[l - 1], off[l])).  Levels count the cut-offs in order of strictness."""
    c, k = _cutoff_array(cutoffs)
    off = np.zeros(max(1, k) + 1, dtype=np.uint64)
    _check(lib().ksp_debug_sweep_bands(device, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col),
                                       c.ctypes.data if c is not None and k else None, k, d_level_ptr or None, off.ctypes.data,
                                       d_a_ptr or None, d_b_ptr or None))
    return off[:k + 1]


def edges_forest(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 5, device: int = 0,
                 tail: int = 0, fill: int = 0) -> np.ndarray:
    """The record indices of the maximum spanning forest of ksp_edge records in DEVICE memory, in merge order (NaN first, then
    value descending, then lower index): the single-linkage tree of the graph (include/kspider_amd.h).  tail / fill (tests): that
    many entries of `fill` are kept behind the room the call may use and checked to be untouched."""
    room = max(0, min(n_nodes - 1, n_edges))
    out = np.full(room + tail, fill, dtype=np.uint32)
    n = ctypes.c_uint32(0xFFFFFFFF)
    _check(lib().ksp_edges_forest(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col),
                                  out.ctypes.data if (room + tail) else None, ctypes.byref(n)))
    if n.value > room or (out[n.value:] != fill).any() and tail:
        raise AssertionError("ksp_edges_forest wrote behind its forest")
    return out[:n.value].copy()


def forest_ranked(n_nodes: int, a: np.ndarray, b: np.ndarray, rank: np.ndarray, device: int = 0, tail: int = 0, fill: int = 0) -> np.ndarray:
    """The same forest for host edges whose weights are already ranked: a higher rank merges earlier, ties go to the lower index."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    if not (a.size == b.size == rank.size):
        raise ValueError("a, b and rank need one entry per edge")
    room = max(0, min(n_nodes - 1, a.size))
    out = np.full(room + tail, fill, dtype=np.uint32)
    n = ctypes.c_uint32(0xFFFFFFFF)
    _check(lib().ksp_forest_ranked(device, n_nodes, a.ctypes.data, b.ctypes.data, rank.ctypes.data, a.size,
                                   out.ctypes.data if (room + tail) else None, ctypes.byref(n)))
    if n.value > room or (out[n.value:] != fill).any() and tail:
        raise AssertionError("ksp_forest_ranked wrote behind its forest")
    return out[:n.value].copy()


def tree(index_prefix: str, dist_type: str = "max_cont", newick: bool = False) -> None:
    """The single-linkage tree of the pairwise TSV: PREFIX_kSpider_tree_<DIST>.tsv, one row per merge (and .newick), from the
    maximum spanning forest the device finds; `cluster_from_tree` then writes the cluster file of any cut-off from it."""
    _check(lib().kspider_tree(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, int(bool(newick))))


def pairwise_and_tree(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", newick: bool = False) -> None:
    """`pairwise` plus the tree files of `tree`, the forest taken from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_tree(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                           int(bool(newick))))


def edges_dereplicate(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 4, threshold: float = 0.20,
                      device: int = 0, tail: int = 0, fill: int = 0) -> dict:
    """The dereplicated set of ksp_edge records in DEVICE memory (include/kspider_amd.h): {"rep", "via", "rank", "degree"}, one entry
    per node, and "n_reps".  rep[v] == v: v is a representative (via[v] = 0xFFFFFFFF); otherwise rep[v] stands for v through record
    via[v].  tail / fill (tests): that many entries of `fill` are kept behind every array and checked to be untouched."""
    out = {k: np.full(n_nodes + tail, fill, dtype=np.uint32) for k in ("rep", "via", "rank", "degree")}
    n = ctypes.c_uint32(0xFFFFFFFF)
    _check(lib().ksp_edges_dereplicate(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), float(threshold),
                                       *[out[k].ctypes.data if (n_nodes + tail) else None for k in ("rep", "via", "rank", "degree")], ctypes.byref(n)))
    for k, a in out.items():
        if tail and (a[n_nodes:] != fill).any():
            raise AssertionError(f"ksp_edges_dereplicate wrote behind {k}")
    res = {k: a[:n_nodes].copy() for k, a in out.items()}
    res["n_reps"] = int(n.value)
    return res


def derep_rounds() -> dict:
    """(tests) What the last dereplication of this thread did (ksp_debug_derep_rounds, csrc/engine_internal.h): the rounds the host
    dispatched, the rounds of the single-workgroup tail (0: it did not run), the live pairs when it took over, the records kept as pairs."""
    out = np.zeros(4, dtype=np.uint64)
    _check(lib().ksp_debug_derep_rounds(out.ctypes.data))
    return dict(dispatched=int(out[0]), tail=int(out[1]), live_at_tail=int(out[2]), kept=int(out[3]))


def dereplicate(index_prefix: str, dist_type: str = "avg_cont", threshold: float = 0.20, out_path: str | None = None) -> None:
    """The dereplicated set of the pairwise TSV: PREFIX_kSpider_dereplicated_<DIST>.tsv (or out_path), one row per source of .namesMap
    with its representative, the value of the row that assigns it, its neighbour count and its rank; the selection runs on the GPU."""
    _check(lib().kspider_dereplicate(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, float(threshold),
                                     os.fsencode(out_path) if out_path else None))


def pairwise_and_dereplicate(index_prefix: str, user_threads: int = 1, dist_type: str = "avg_cont", threshold: float = 0.20,
                             out_path: str | None = None) -> None:
    """`pairwise` plus the file of `dereplicate`, the selection taken from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_dereplicate(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                                  float(threshold), os.fsencode(out_path) if out_path else None))


def _topk_k(k) -> int:
    k = int(k)
    if not 0 <= k <= 0xFFFFFFFF:
        raise ValueError("k does not fit 32 bits")
    return k


def _topk_out(who, n_nodes, k, tail, fill, call):
    room = n_nodes * k
    index = np.full(room + tail, fill, dtype=np.uint32)
    count = np.full(n_nodes + tail, fill, dtype=np.uint32)
    _check(call(index.ctypes.data if (room + tail) else None, count.ctypes.data if (n_nodes + tail) else None))
    if tail and ((index[room:] != fill).any() or (count[n_nodes:] != fill).any()):
        raise AssertionError(f"{who} wrote behind its arrays")
    return index[:room].reshape(n_nodes, k).copy(), count[:n_nodes].copy()


def edges_topk(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 5, k: int = 5, device: int = 0,
               tail: int = 0, fill: int = 0) -> tuple:
    """The k best hits of every node among ksp_edge records in DEVICE memory (include/kspider_amd.h): (index, count), index[v, i] for
    i < count[v] the record index of the i-th entry of v by (value descending, NaN last, lower index first), 0xFFFFFFFF behind.
    tail / fill (tests): that many entries of `fill` are kept behind both arrays and checked to be untouched."""
    k = _topk_k(k)
    return _topk_out("ksp_edges_topk", n_nodes, k, tail, fill, lambda pi, pc: lib().ksp_edges_topk(
        device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), k, pi, pc))


def topk_ranked(n_nodes: int, a: np.ndarray, b: np.ndarray, rank: np.ndarray, k: int = 5, device: int = 0, tail: int = 0, fill: int = 0) -> tuple:
    """The same selection for host edges whose values are already ranked: a higher rank is better, ties go to the lower index."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    rank = np.ascontiguousarray(rank, dtype=np.uint32)
    if not (a.size == b.size == rank.size):
        raise ValueError("a, b and rank need one entry per edge")
    k = _topk_k(k)
    return _topk_out("ksp_topk_ranked", n_nodes, k, tail, fill, lambda pi, pc: lib().ksp_topk_ranked(
        device, n_nodes, a.ctypes.data, b.ctypes.data, rank.ctypes.data, a.size, k, pi, pc))


def topk_classes() -> dict:
    """(tests) What the last top-k selection of this thread did (ksp_debug_topk_classes, csrc/engine_internal.h): the nodes selected by
    the wave, workgroup and stream kernels, and the refills of the stream kernel over all its nodes."""
    out = np.zeros(4, dtype=np.uint64)
    _check(lib().ksp_debug_topk_classes(out.ctypes.data))
    return dict(wave=int(out[0]), workgroup=int(out[1]), stream=int(out[2]), refills=int(out[3]))


def topk(index_prefix: str, dist_type: str = "max_cont", k: int = 5, out_path: str | None = None) -> None:
    """The k best hits of every source of the pairwise TSV: PREFIX_kSpider_topk_<DIST>.tsv (or out_path), one row per hit with both
    names of .namesMap and the value as it stands in the TSV; the selection runs on the GPU."""
    _check(lib().kspider_topk(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, _topk_k(k),
                              os.fsencode(out_path) if out_path else None))


def pairwise_and_topk(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", k: int = 5, out_path: str | None = None) -> None:
    """`pairwise` plus the file of `topk`, the selection taken from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_topk(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                           _topk_k(k), os.fsencode(out_path) if out_path else None))


def _report_out(who, n_nodes, tail, fill, call):
    """Both outputs of a report call with `tail` rows of the byte `fill` behind them (all n_nodes rows of the cluster array start as
    `fill` too).  After a refused call (KspError) every byte is checked to be untouched; after a good one the rows behind n_clusters
    and both tails are."""
    cluster = np.full((n_nodes + tail) * CLUSTER_ROW_DTYPE.itemsize, fill, dtype=np.uint8)
    member = np.full((n_nodes + tail) * MEMBER_ROW_DTYPE.itemsize, fill, dtype=np.uint8)
    n_clusters = np.full(1 + tail, fill * 0x01010101, dtype=np.uint32)
    try:
        _check(call(cluster.ctypes.data if cluster.size else None, n_clusters.ctypes.data, member.ctypes.data if member.size else None))
    except KspError:
        if (cluster != fill).any() or (member != fill).any() or (n_clusters != fill * 0x01010101).any():
            raise AssertionError(f"{who} wrote to its outputs although it refused the call")
        raise
    n = int(n_clusters[0])
    if n > n_nodes:
        raise AssertionError(f"{who} reported more clusters than nodes")
    if (cluster[n * CLUSTER_ROW_DTYPE.itemsize:] != fill).any() or (member[n_nodes * MEMBER_ROW_DTYPE.itemsize:] != fill).any() or (n_clusters[1:] != fill * 0x01010101).any():
        raise AssertionError(f"{who} wrote behind its rows")
    return (cluster[:n * CLUSTER_ROW_DTYPE.itemsize].view(CLUSTER_ROW_DTYPE).copy(), member[:n_nodes * MEMBER_ROW_DTYPE.itemsize].view(MEMBER_ROW_DTYPE).copy())


def edges_cluster_report(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 5, cutoff: float = 0.0, device: int = 0,
                         tail: int = 0, fill: int = 0) -> tuple:
    """The report of every cluster of the kept ksp_edge records in DEVICE memory (include/kspider_amd.h): (cluster, member), structured
    arrays of CLUSTER_ROW_DTYPE (one row per cluster, by root) and MEMBER_ROW_DTYPE (one row per node).  tail / fill (tests): that many
    rows of the byte `fill` are kept behind both arrays and checked to be untouched, as are the cluster rows behind the last one."""
    return _report_out("ksp_edges_cluster_report", n_nodes, tail, fill, lambda pc, pn, pm: lib().ksp_edges_cluster_report(
        device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), float(cutoff), pc, pn, pm))


def cluster_report_valued(n_nodes: int, a: np.ndarray, b: np.ndarray, value: np.ndarray, device: int = 0, tail: int = 0, fill: int = 0) -> tuple:
    """The same report for host edges the caller has cut already: every record is kept, value[e] in [0, 1] or NaN."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    value = np.ascontiguousarray(value, dtype=np.float32)
    if not (a.size == b.size == value.size):
        raise ValueError("a, b and value need one entry per edge")
    return _report_out("ksp_cluster_report_valued", n_nodes, tail, fill, lambda pc, pn, pm: lib().ksp_cluster_report_valued(
        device, n_nodes, a.ctypes.data, b.ctypes.data, value.ctypes.data, a.size, pc, pn, pm))


def report_counts() -> dict:
    """(tests) What the last report of this thread did (ksp_debug_report_counts, csrc/engine_internal.h): the kept records, the chunks
    that took the single-label path, the sets of cluster atomics and of source_1-side node atomics issued."""
    out = np.zeros(4, dtype=np.uint64)
    _check(lib().ksp_debug_report_counts(out.ctypes.data))
    return dict(kept=int(out[0]), single_label_chunks=int(out[1]), cluster_sets=int(out[2]), node_sets=int(out[3]))


def cluster_report(index_prefix: str, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """The report of every cluster of the pairwise TSV at one cut-off: PREFIX_kSpider_cluster_report_<DIST>_<CUTOFF*100>%.tsv and
    PREFIX_kSpider_cluster_members_<DIST>_<CUTOFF*100>%.tsv; the sums run on the GPU."""
    _check(lib().kspider_cluster_report(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, float(cutoff)))


def pairwise_and_cluster_report(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """`pairwise` plus the two files of `cluster_report`, the report taken from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_cluster_report(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                                     float(cutoff)))


def _upgma_out(who, n_nodes, tail, fill, call):
    """The rows of an UPGMA call with `tail` rows of the byte `fill` behind the room for n_nodes - 1 rows (which starts as `fill` too).
    After a refused call (KspError) every byte is checked to be untouched; after a good one the rows behind n_rows are."""
    room = max(0, n_nodes - 1)
    rows = np.full((room + tail) * UPGMA_ROW_DTYPE.itemsize, fill, dtype=np.uint8)
    n_rows = np.full(1 + tail, fill * 0x01010101, dtype=np.uint32)
    try:
        _check(call(rows.ctypes.data if rows.size else None, n_rows.ctypes.data))
    except KspError:
        if (rows != fill).any() or (n_rows != fill * 0x01010101).any():
            raise AssertionError(f"{who} wrote to its outputs although it refused the call")
        raise
    n = int(n_rows[0])
    if n > room:
        raise AssertionError(f"{who} reported more merges than a forest has")
    if (rows[n * UPGMA_ROW_DTYPE.itemsize:] != fill).any() or (n_rows[1:] != fill * 0x01010101).any():
        raise AssertionError(f"{who} wrote behind its rows")
    return rows[:n * UPGMA_ROW_DTYPE.itemsize].view(UPGMA_ROW_DTYPE).copy()


def edges_upgma(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, dist_col: int = 5, device: int = 0, tail: int = 0,
                fill: int = 0) -> np.ndarray:
    """The exact average-linkage (UPGMA) merges of ksp_edge records in DEVICE memory (include/kspider_amd.h), in merge order: a structured
    array of UPGMA_ROW_DTYPE.  tail / fill (tests): that many rows of the byte `fill` are kept behind the room the call may use and
    checked to be untouched, as are the rows behind the last one."""
    return _upgma_out("ksp_edges_upgma", n_nodes, tail, fill, lambda pr, pn: lib().ksp_edges_upgma(
        device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(dist_col), pr, pn))


def upgma_valued(n_nodes: int, a: np.ndarray, b: np.ndarray, value: np.ndarray, device: int = 0, tail: int = 0, fill: int = 0) -> np.ndarray:
    """The same merges for host edges the caller has valued already: value[e] in [0, 1] or NaN (takes no part)."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    value = np.ascontiguousarray(value, dtype=np.float32)
    if not (a.size == b.size == value.size):
        raise ValueError("a, b and value need one entry per edge")
    return _upgma_out("ksp_upgma_valued", n_nodes, tail, fill, lambda pr, pn: lib().ksp_upgma_valued(
        device, n_nodes, a.ctypes.data, b.ctypes.data, value.ctypes.data, a.size, pr, pn))


def upgma_before(pair1, pair2) -> bool:
    """Host only: does candidate pair 1 come before pair 2 in the order of the average-linkage tree?  A pair is
    (sum_q, size_lo, size_hi, lo, hi); the similarities sum_q / (size_lo * size_hi) are compared exactly."""
    out = ctypes.c_int(-1)
    _check(lib().ksp_upgma_before(*[int(x) for x in pair1], *[int(x) for x in pair2], ctypes.byref(out)))
    return bool(out.value)


def upgma_counts() -> dict:
    """(tests) What the last UPGMA call of this thread did (ksp_debug_upgma_counts, csrc/engine_internal.h)."""
    out = np.zeros(6, dtype=np.uint64)
    _check(lib().ksp_debug_upgma_counts(out.ctypes.data))
    return dict(first_pairs=int(out[0]), rounds=int(out[1]), device_merges=int(out[2]), handed_over=int(out[3]), host_merges=int(out[4]),
                longest_run=int(out[5]))


def upgma(index_prefix: str, dist_type: str = "max_cont", newick: bool = False) -> None:
    """The average-linkage tree (UPGMA) of the pairwise TSV: PREFIX_kSpider_upgma_<DIST>.tsv, one row per merge (and .newick), the
    merges found on the GPU from the sparse rows; `cluster_from_upgma` then writes the clusters of any cut-off from it."""
    _check(lib().kspider_upgma(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, int(bool(newick))))


def pairwise_and_upgma(index_prefix: str, user_threads: int = 1, dist_type: str = "max_cont", newick: bool = False) -> None:
    """`pairwise` plus the files of `upgma`, the merges taken from the edges while they are in HBM."""
    _check(lib().kspider_pairwise_and_upgma(os.fsencode(index_prefix), int(user_threads), dist_type.encode() if dist_type is not None else None,
                                            int(bool(newick))))


def cluster_from_upgma(index_prefix: str, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """The clusters of the average-linkage tree at one cut-off, from PREFIX_kSpider_upgma_<DIST>.tsv alone (host only):
    PREFIX_kSpider_clusters_upgma_<DIST>_<CUTOFF*100>%.tsv in the format of `cluster`."""
    _check(lib().kspider_cluster_from_upgma(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, float(cutoff)))


def edges_tsv(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, d_ids_ptr: int = 0, device: int = 0, capacity: int | None = None,
              tail: int = 0, fill: int = 0xA5) -> bytes:
    """The rows of the pairwise TSV for ksp_edge records in DEVICE memory, as text made on the device (ksp_edges_tsv in
    include/kspider_amd.h): no header, the records' order, ids from the device array d_ids_ptr (0: the source indices themselves).
    capacity None: the size query first, then a buffer of exactly that size.  tail / fill (tests): that many bytes of `fill` are
    kept behind the text and checked to be untouched; after a refused call (KspError) the whole buffer is checked."""
    n = ctypes.c_uint64(0)
    args = (device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, d_ids_ptr or None)
    if capacity is None:
        _check(lib().ksp_edges_tsv(*args, None, 0, ctypes.byref(n)))
        capacity = n.value
    buf = np.full(capacity + tail, fill, dtype=np.uint8)
    rc = lib().ksp_edges_tsv(*args, buf.ctypes.data, capacity, ctypes.byref(n))
    written = n.value if rc == KSP_OK else 0
    if (buf[written:] != fill).any():
        raise AssertionError("ksp_edges_tsv wrote behind its text" if rc == KSP_OK else "ksp_edges_tsv refused the call and wrote all the same")
    _check(rc)
    return buf[:written].tobytes()


def edges_tsv_size(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, d_ids_ptr: int = 0, device: int = 0) -> int:
    """The bytes edges_tsv would return (ksp_edges_tsv with h_text = NULL)."""
    n = ctypes.c_uint64(0)
    _check(lib().ksp_edges_tsv(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, d_ids_ptr or None, None, 0, ctypes.byref(n)))
    return n.value


def _float_texts(call, values, raw):
    v = np.ascontiguousarray(values, dtype=np.float32).ravel()
    text = np.zeros((v.size, 16), dtype=np.uint8)
    length = np.zeros(v.size, dtype=np.uint32)
    _check(call(v.ctypes.data if v.size else None, v.size, text.ctypes.data if v.size else None, length.ctypes.data if v.size else None))
    if v.size and int(length.max()) > 16:
        raise AssertionError("a text longer than its 16-byte slot")
    if raw:
        return text, length
    data = text.tobytes()
    return [data[16 * i:16 * i + int(n)].decode("ascii") for i, n in enumerate(length)]


def format_floats_device(values, device: int = 0, raw: bool = False):
    """(tests) The text of every float32 of `values` as the device prints it (ksp_debug_format_floats, csrc/engine_internal.h): what
    format_float gives, from integer arithmetic.  A list of str, or with raw (text, length): an (n, 16) uint8 array whose row i
    holds length[i] bytes of text and zeros behind.  KspError (KSP_E_ARG) when a value is outside 0, +inf and [2^-40, 2^40)."""
    return _float_texts(lambda v, n, t, l: lib().ksp_debug_format_floats(device, v, n, t, l), values, raw)


def format_floats(values, raw: bool = False):
    """format_float of every float32 of `values` in one call (ksp_debug_format_floats_host): the same host snprintf, the layout of
    format_floats_device."""
    return _float_texts(lambda v, n, t, l: lib().ksp_debug_format_floats_host(v, n, t, l), values, raw)


def tsv_records(n_nodes: int, n_edges: int, seed: int, d_edges_ptr: int, d_kmer_counts_ptr: int, d_ids_ptr: int, device: int = 0) -> None:
    """(tools/tsv_times.py) ksp_debug_tsv_records: valid seeded records, k-mer counts and ids written into the caller's device arrays."""
    _check(lib().ksp_debug_tsv_records(device, n_nodes, n_edges, seed, d_edges_ptr or None, d_kmer_counts_ptr or None, d_ids_ptr or None))


def tsv_times(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, d_ids_ptr: int, which: int, reps: int, threads: int = 16,
              device: int = 0) -> np.ndarray:
    """(tools/tsv_times.py) ksp_debug_tsv_times: reps rows of (wall ms, which 0: kernel ms by HIP events / which 1: ms of the copy)."""
    ms = np.zeros((reps, 2), dtype=np.float32)
    _check(lib().ksp_debug_tsv_times(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, d_ids_ptr or None, int(which), int(reps),
                                     int(threads), ms.ctypes.data))
    return ms


def _ptr(a):
    """Address of a numpy array, or None for None (the C side's NULL)."""
    return None if a is None else a.ctypes.data


def _u64(a):
    """A contiguous uint64 array, or None for None."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint64)


def _n_sketches(offsets):
    """The sketches an offsets array describes: one fewer than its entries, 0 for None or an empty one."""
    return 0 if offsets is None else max(offsets.size - 1, 0)


def _take(out, count, dtype):
    """`count` items of `dtype` at the C buffer `out` (a c_void_p) as a numpy copy; the buffer is freed whether the copy succeeds or not."""
    try:
        buf = (ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(out.value) if count else b""
        return np.frombuffer(buf, dtype=dtype).copy()
    finally:
        lib().ksp_free(out)


def query_host(db_keys, db_offsets, q_keys, q_offsets, mode: int = QUERY_CROSS, device: int = 0):
    """Host sketches of a database and of queries -> (edges sorted by (source_1, source_2), stats).  Database sources are numbered
    0 .. n_db - 1, queries n_db .. n_db + n_q - 1; mode QUERY_CROSS: database x query pairs, QUERY_CROSS_AND_SELF: also query x
    query.  None stands for a NULL pointer (refused by the C side)."""
    dk, do, qk, qo = _u64(db_keys), _u64(db_offsets), _u64(q_keys), _u64(q_offsets)
    out = ctypes.c_void_p()
    ne = ctypes.c_uint64(0)
    st = QueryStats()
    _check(lib().ksp_query_host(_ptr(dk), _ptr(do), _n_sketches(do), _ptr(qk), _ptr(qo), _n_sketches(qo),
                                int(mode), int(device), ctypes.byref(out), ctypes.byref(ne), ctypes.byref(st)))
    edges = _take(out, ne.value, EDGE_DTYPE)
    return edges, st.as_dict()


def query_device(d_db_keys_ptr: int, db_offsets, d_q_keys_ptr: int, q_offsets, d_edges_ptr: int, capacity: int, mode: int = QUERY_CROSS, device: int = 0) -> tuple:
    """ksp_query_device: keys in DEVICE memory, offsets on the host, edges into d_edges (room for `capacity`; 0 / 0: the size query).
    -> (rc, n_edges, stats): rc is KSP_OK or KSP_E_OVERFLOW (n_edges is then the required size); anything else raises."""
    do, qo = _u64(db_offsets), _u64(q_offsets)
    ne = ctypes.c_uint64(0)
    st = QueryStats()
    rc = lib().ksp_query_device(int(device), d_db_keys_ptr or None, _ptr(do), _n_sketches(do), d_q_keys_ptr or None, _ptr(qo),
                                _n_sketches(qo), int(mode), d_edges_ptr or None, int(capacity), ctypes.byref(ne), ctypes.byref(st))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    return rc, ne.value, st.as_dict()


def query_directory(max_key: int, n_keys: int) -> tuple:
    """(bits, shift) of the first level of a query table of n_keys distinct keys, the largest max_key (host only)."""
    bits, shift = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().ksp_query_directory(int(max_key), int(n_keys), ctypes.byref(bits), ctypes.byref(shift)))
    return bits.value, shift.value


def pack(sketch_dir: str, kSize: int, out_path: str, user_threads: int = 1) -> None:
    """A directory of .sig / .gz files (kSize > 0) or .bin files (kSize = 0) -> one pack file (kspider_pack)."""
    _check(lib().kspider_pack(os.fsencode(sketch_dir), int(kSize), os.fsencode(out_path), int(user_threads)))


def pack_read(path: str) -> dict:
    """A pack file, read whole and checked (ksp_pack_info + ksp_pack_load; host only): ksize, names (one per group), present and
    kmers per group, offsets and keys of the groups that have a sketch."""
    info = np.zeros(5, dtype=np.uint64)
    _check(lib().ksp_pack_info(os.fsencode(path), info.ctypes.data))
    ksize, G, S, K, B = int(np.int64(info[0])), int(info[1]), int(info[2]), int(info[3]), int(info[4])
    kmers, present = np.zeros(G + 1, dtype=np.uint32), np.zeros(G + 1, dtype=np.uint8)
    offsets, keys, name_off = np.zeros(S + 1, dtype=np.uint64), np.zeros(K + 1, dtype=np.uint64), np.zeros(G + 1, dtype=np.uint64)
    text = np.zeros(B + 1, dtype=np.uint8)
    _check(lib().ksp_pack_load(os.fsencode(path), kmers.ctypes.data, present.ctypes.data, offsets.ctypes.data, keys.ctypes.data, name_off.ctypes.data,
                               text.ctypes.data))
    blob = text[:B].tobytes()
    names = [os.fsdecode(blob[int(name_off[g]):int(name_off[g + 1])]) for g in range(G)]
    return {"ksize": ksize, "names": names, "present": present[:G].copy(), "kmers": kmers[:G].copy(), "offsets": offsets, "keys": keys[:K].copy()}


def query(db: str, queries: str, kSize: int, out_prefix: str, user_threads: int = 1, mode: int = QUERY_CROSS) -> None:
    """New sketches against a database (kspider_query): db and queries are each a pack file or a directory; writes OUT.namesMap,
    OUT_kSpider_seqToKmersNo.tsv and OUT_kSpider_pairwise.tsv with only the rows of the mode."""
    _check(lib().kspider_query(os.fsencode(db), os.fsencode(queries), int(kSize), os.fsencode(out_prefix) if out_prefix else None, int(user_threads), int(mode)))


def gather_host(db_keys, db_offsets, q_keys, q_offsets, min_hashes: int = 1, max_matches: int = 0, device: int = 0):
    """What every query is made of (ksp_gather_host): host sketches of a database and of queries -> (rows ordered by (query, rank),
    stats).  A row (GATHER_ROW_DTYPE) names the database source that covers most of what is left of the query, its overlap with the
    whole query, the hashes it was the first to cover (unique) and what remains after it; a source is reported while unique is at
    least min_hashes; max_matches caps the rows per query (0: no cap).  None stands for a NULL pointer (refused by the C side)."""
    dk, do, qk, qo = _u64(db_keys), _u64(db_offsets), _u64(q_keys), _u64(q_offsets)
    out = ctypes.c_void_p()
    nr = ctypes.c_uint64(0)
    st = GatherStats()
    _check(lib().ksp_gather_host(_ptr(dk), _ptr(do), _n_sketches(do), _ptr(qk), _ptr(qo), _n_sketches(qo),
                                 int(min_hashes), int(max_matches), int(device), ctypes.byref(out), ctypes.byref(nr), ctypes.byref(st)))
    rows = _take(out, nr.value, GATHER_ROW_DTYPE)
    return rows, st.as_dict()


def gather_device(d_db_keys_ptr: int, db_offsets, d_q_keys_ptr: int, q_offsets, d_rows_ptr: int, capacity: int, min_hashes: int = 1, max_matches: int = 0,
                  device: int = 0) -> tuple:
    """ksp_gather_device: keys in DEVICE memory, offsets on the host, rows into d_rows (room for `capacity`; 0 / 0: the size query).
    -> (rc, n_rows, stats): rc is KSP_OK or KSP_E_OVERFLOW (n_rows is then the required size); anything else raises."""
    do, qo = _u64(db_offsets), _u64(q_offsets)
    nr = ctypes.c_uint64(0)
    st = GatherStats()
    rc = lib().ksp_gather_device(int(device), d_db_keys_ptr or None, _ptr(do), _n_sketches(do), d_q_keys_ptr or None, _ptr(qo),
                                 _n_sketches(qo), int(min_hashes), int(max_matches), d_rows_ptr or None, int(capacity), ctypes.byref(nr),
                                 ctypes.byref(st))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    return rc, nr.value, st.as_dict()


def gather(db: str, queries: str, kSize: int, out_prefix: str, user_threads: int = 1, min_hashes: int = 1, max_matches: int = 0) -> None:
    """What every query sketch is made of (kspider_gather): db and queries are each a pack file or a directory; writes
    OUT_kSpider_gather.tsv."""
    _check(lib().kspider_gather(os.fsencode(db), os.fsencode(queries), int(kSize), os.fsencode(out_prefix) if out_prefix else None, int(user_threads),
                                int(min_hashes), int(max_matches)))


def gather_abund_host(db_keys, db_offsets, q_keys, q_abund, q_offsets, min_hashes: int = 1, max_matches: int = 0, device: int = 0):
    """gather_host for queries that carry an abundance per hash (ksp_gather_abund_host): q_abund is parallel to q_keys -> (rows of
    GATHER_WROW_DTYPE, stats).  The first six fields are gather_host's; w_unique, w_found, the 128-bit sum of squares and twice the
    median are over the hashes a row takes, with the query's abundances."""
    dk, do, qk, qo = _u64(db_keys), _u64(db_offsets), _u64(q_keys), _u64(q_offsets)
    qa = None if q_abund is None else np.ascontiguousarray(q_abund, dtype=np.uint32)
    out = ctypes.c_void_p()
    nr = ctypes.c_uint64(0)
    st = GatherStats()
    _check(lib().ksp_gather_abund_host(_ptr(dk), _ptr(do), _n_sketches(do), _ptr(qk), _ptr(qa), _ptr(qo), _n_sketches(qo),
                                       int(min_hashes), int(max_matches), int(device), ctypes.byref(out), ctypes.byref(nr), ctypes.byref(st)))
    rows = _take(out, nr.value, GATHER_WROW_DTYPE)
    return rows, st.as_dict()


def gather_abund_device(d_db_keys_ptr: int, db_offsets, d_q_keys_ptr: int, d_q_abund_ptr: int, q_offsets, d_rows_ptr: int, capacity: int, min_hashes: int = 1,
                        max_matches: int = 0, device: int = 0) -> tuple:
    """ksp_gather_abund_device: keys and abundances in DEVICE memory, offsets on the host, rows of 64 bytes into d_rows (room for
    `capacity`; 0 / 0: the size query).  -> (rc, n_rows, stats) as gather_device."""
    do, qo = _u64(db_offsets), _u64(q_offsets)
    nr = ctypes.c_uint64(0)
    st = GatherStats()
    rc = lib().ksp_gather_abund_device(int(device), d_db_keys_ptr or None, _ptr(do), _n_sketches(do), d_q_keys_ptr or None, d_q_abund_ptr or None,
                                       _ptr(qo), _n_sketches(qo), int(min_hashes), int(max_matches), d_rows_ptr or None, int(capacity),
                                       ctypes.byref(nr), ctypes.byref(st))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    return rc, nr.value, st.as_dict()


def gather_abund(db: str, queries: str, kSize: int, out_prefix: str, user_threads: int = 1, min_hashes: int = 1, max_matches: int = 0) -> None:
    """kspider_gather_abund: gather for a directory of query signatures with abundances; OUT_kSpider_gather.tsv has gather's nine
    columns, then f_unique_weighted, average_abund, median_abund, std_abund, n_unique_weighted_found, sum_weighted_found and
    total_weighted_hashes."""
    _check(lib().kspider_gather_abund(os.fsencode(db), os.fsencode(queries), int(kSize), os.fsencode(out_prefix) if out_prefix else None, int(user_threads),
                                      int(min_hashes), int(max_matches)))


def _u32(a):
    """A contiguous uint32 array, or None for None."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.uint32)


def compare_host(db_keys, db_abund, db_offsets, q_keys, q_abund, q_offsets, mode: int = QUERY_CROSS_AND_SELF, device: int = 0):
    """Counted sketches against each other (ksp_compare_host) -> (rows of WEDGE_DTYPE sorted by (source_1, source_2), sum, sumsq,
    stats).  Sources are numbered as in query_host; an abundance array is parallel to its keys, None stands for all ones.  With
    mode QUERY_CROSS_AND_SELF the database may be None, None, None: every pair of the queries.  sum / sumsq: per source, Σ a and
    Σ a² as uint64 (a source with Σ a² >= 2^64 is refused with KSP_E_LIMIT)."""
    dk, do, qk, qo = _u64(db_keys), _u64(db_offsets), _u64(q_keys), _u64(q_offsets)
    da, qa = _u32(db_abund), _u32(q_abund)
    n = _n_sketches(do) + _n_sketches(qo)
    total, sq = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    out = ctypes.c_void_p()
    nr = ctypes.c_uint64(0)
    st = CompareStats()
    _check(lib().ksp_compare_host(_ptr(dk), _ptr(da), _ptr(do), _n_sketches(do), _ptr(qk), _ptr(qa), _ptr(qo), _n_sketches(qo), int(mode), int(device),
                                  ctypes.byref(out), ctypes.byref(nr), total.ctypes.data, sq.ctypes.data, ctypes.byref(st)))
    rows = _take(out, nr.value, WEDGE_DTYPE)
    return rows, total[:n].copy(), sq[:n].copy(), st.as_dict()


def compare_device(d_db_keys_ptr: int, d_db_abund_ptr: int, db_offsets, d_q_keys_ptr: int, d_q_abund_ptr: int, q_offsets, d_rows_ptr: int, capacity: int,
                   mode: int = QUERY_CROSS_AND_SELF, device: int = 0) -> tuple:
    """ksp_compare_device: keys and abundances in DEVICE memory (an abundance pointer of 0 / None: all ones), offsets on the host,
    rows of 40 bytes into d_rows (room for `capacity`; 0 / 0: the size query).  -> (rc, n_rows, sum, sumsq, stats): rc is KSP_OK or
    KSP_E_OVERFLOW (n_rows is then the required size); anything else raises."""
    do, qo = _u64(db_offsets), _u64(q_offsets)
    n = _n_sketches(do) + _n_sketches(qo)
    total, sq = np.zeros(n + 1, dtype=np.uint64), np.zeros(n + 1, dtype=np.uint64)
    nr = ctypes.c_uint64(0)
    st = CompareStats()
    rc = lib().ksp_compare_device(int(device), d_db_keys_ptr or None, d_db_abund_ptr or None, _ptr(do), _n_sketches(do), d_q_keys_ptr or None, d_q_abund_ptr or None,
                                  _ptr(qo), _n_sketches(qo), int(mode), d_rows_ptr or None, int(capacity), ctypes.byref(nr), total.ctypes.data, sq.ctypes.data,
                                  ctypes.byref(st))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    return rc, nr.value, total[:n].copy(), sq[:n].copy(), st.as_dict()


def compare_values(row, n_1: int, sum_1: int, sumsq_1: int, n_2: int, sum_2: int, sumsq_2: int) -> tuple:
    """(cosine, angular similarity, weighted containment 1, weighted containment 2) of a row (a WEDGE_DTYPE record or a tuple of
    its six fields) and the totals of its two sources (ksp_compare_values; host only)."""
    w = Wedge(*(int(x) for x in (row.tolist() if hasattr(row, "tolist") else row)))
    out = (ctypes.c_double * 4)()
    _check(lib().ksp_compare_values(ctypes.byref(w), int(n_1), int(sum_1), int(sumsq_1), int(n_2), int(sum_2), int(sumsq_2), out))
    return tuple(out)


def compare(samples: str, kSize: int, out_prefix: str, user_threads: int = 1, against: str | None = None, matrix: bool = False) -> None:
    """kspider_compare: every pair of the sample signatures in a directory — or, with `against` (a directory or a pack file), every
    database source against every sample — as OUT_kSpider_compare.tsv beside OUT.namesMap and OUT_kSpider_seqToKmersNo.tsv; matrix
    (without `against`): also OUT_kSpider_compare_matrix.csv, the N x N angular similarities."""
    _check(lib().kspider_compare(os.fsencode(samples) if samples else None, os.fsencode(against) if against else None, int(kSize),
                                 os.fsencode(out_prefix) if out_prefix else None, int(user_threads), COMPARE_MATRIX if matrix else 0))


def sig_read(path: str, kSize: int) -> tuple:
    """One .sig / .sig.gz file as the loaders read it (ksp_sig_read; host only) -> (mins sorted and distinct, abundances parallel to
    them or None when the signature has none)."""
    n, has = ctypes.c_uint64(0), ctypes.c_int(0)
    rc = lib().ksp_sig_read(os.fsencode(path), int(kSize), None, None, 0, ctypes.byref(n), ctypes.byref(has))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    mins, abunds = np.zeros(max(n.value, 1), dtype=np.uint64), np.zeros(max(n.value, 1), dtype=np.uint32)
    _check(lib().ksp_sig_read(os.fsencode(path), int(kSize), mins.ctypes.data, abunds.ctypes.data, n.value, ctypes.byref(n), ctypes.byref(has)))
    return mins[:n.value].copy(), (abunds[:n.value].copy() if has.value else None)


def sketch_max_hash(scaled: int) -> int:
    """sourmash's threshold of `scaled` (host only): 2^64 - 1 for 1, int(2^64 / float(scaled)) above; 0 is refused."""
    out = ctypes.c_uint64(0)
    _check(lib().ksp_sketch_max_hash(int(scaled), ctypes.byref(out)))
    return out.value


def murmur64(data: bytes, seed: int = 42) -> tuple:
    """Both words of MurmurHash3_x64_128 over the bytes (host only)."""
    data = bytes(data)
    out = np.zeros(2, dtype=np.uint64)
    _check(lib().ksp_murmur64(data, len(data), int(seed), out.ctypes.data))
    return int(out[0]), int(out[1])


def sketch_kmer_hash(text, seed: int = 42) -> tuple:
    """(hash, valid) of the k-mer the bytes spell (host only); valid is False, and hash 0, when a byte is not one of ACGTacgt."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    h, v = ctypes.c_uint64(0), ctypes.c_int(0)
    _check(lib().ksp_sketch_kmer_hash(text, len(text), int(seed), ctypes.byref(h), ctypes.byref(v)))
    return h.value, bool(v.value)


def _sketch_input(seq, src_offsets, max_hash, scaled):
    if (max_hash is None) == (scaled is None):
        raise ValueError("give max_hash or scaled")
    buf = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, dtype=np.uint8)
    off = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    return buf, off, (sketch_max_hash(scaled) if max_hash is None else int(max_hash))


def _sketch_cpu(entry, lead, abund, seq, src_offsets, ksize, max_hash, scaled, seed):
    """A host loop: the size query, then the fill -> (keys, [abund,] offsets).  entry: the C function; lead: its arguments between
    ksize and max_hash; abund: None when it takes no abundance buffer, else whether one is passed and returned."""
    buf, off, mh = _sketch_input(seq, src_offsets, max_hash, scaled)
    n_src = max(off.size - 1, 0)
    out_off = np.zeros(n_src + 1, dtype=np.uint64)
    needed = ctypes.c_uint64(0)

    def call(keys, counts, capacity):
        return entry(_ptr(buf), buf.size, _ptr(off), n_src, int(ksize), *lead, mh, int(seed), _ptr(keys), *(() if abund is None else (_ptr(counts),)), capacity,
                     out_off.ctypes.data, ctypes.byref(needed))

    rc = call(None, None, 0)
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    keys, counts = np.zeros(max(needed.value, 1), dtype=np.uint64), (np.zeros(max(needed.value, 1), dtype=np.uint32) if abund else None)
    _check(call(keys, counts, needed.value))
    return (keys[:needed.value].copy(),) + ((counts[:needed.value].copy(),) if abund else ()) + (out_off,)


def _sketch_host(entry, lead, abund, seq, src_offsets, ksize, max_hash, scaled, seed, device):
    """A call that sketches host bytes on the device and returns malloc'ed buffers -> (keys, [abund,] offsets, stats); the
    arguments as in _sketch_cpu."""
    buf, off, mh = _sketch_input(seq, src_offsets, max_hash, scaled)
    n_src = max(off.size - 1, 0)
    out_off = np.zeros(n_src + 1, dtype=np.uint64)
    out, out_a = ctypes.c_void_p(), ctypes.c_void_p()
    st = SketchStats()
    _check(entry(int(device), _ptr(buf), buf.size, _ptr(off), n_src, int(ksize), *lead, mh, int(seed), ctypes.byref(out),
                 *(() if abund is None else (ctypes.byref(out_a) if abund else None,)), out_off.ctypes.data, ctypes.byref(st)))
    try:
        keys = _take(out, int(out_off[-1]), np.uint64)
    finally:   # (the second buffer is freed also when the first copy failed)
        counts = _take(out_a, int(out_off[-1]), np.uint32) if abund else None
    return (keys,) + ((counts,) if abund else ()) + (out_off, st.as_dict())


def _sketch_device(entry, lead, abund_ptr, d_seq_ptr, n_bytes, src_offsets, ksize, max_hash, d_out_keys_ptr, capacity, seed, device):
    """A call on bytes and keys in DEVICE memory -> (rc, offsets, stats): rc is KSP_OK or KSP_E_OVERFLOW, anything else raises.
    abund_ptr: None when the entry takes no abundance buffer, else its device address (0: NULL); entry and lead as in _sketch_cpu."""
    off = np.ascontiguousarray(src_offsets, dtype=np.uint64)
    n_src = max(off.size - 1, 0)
    out_off = np.zeros(n_src + 1, dtype=np.uint64)
    st = SketchStats()
    rc = entry(int(device), d_seq_ptr or None, int(n_bytes), _ptr(off), n_src, int(ksize), *lead, int(max_hash), int(seed), d_out_keys_ptr or None,
               *(() if abund_ptr is None else (abund_ptr or None,)), int(capacity), out_off.ctypes.data, ctypes.byref(st))
    if rc not in (KSP_OK, KSP_E_OVERFLOW):
        _check(rc)
    return rc, out_off, st.as_dict()


def sketch_cpu(seq, src_offsets, ksize: int, max_hash: int | None = None, scaled: int | None = None, seed: int = 42) -> tuple:
    """ksp_sketch_cpu, the plain host loop: bytes and source offsets -> (keys, offsets) of the sources' sketches.  No GPU."""
    return _sketch_cpu(lib().ksp_sketch_cpu, (), None, seq, src_offsets, ksize, max_hash, scaled, seed)


def sketch_cpu_abund(seq, src_offsets, ksize: int, max_hash: int | None = None, scaled: int | None = None, seed: int = 42) -> tuple:
    """ksp_sketch_cpu_abund: sketch_cpu with every key's abundance -> (keys, abund, offsets).  No GPU."""
    return _sketch_cpu(lib().ksp_sketch_cpu_abund, (), True, seq, src_offsets, ksize, max_hash, scaled, seed)


def sketch_host_abund(seq, src_offsets, ksize: int, max_hash: int | None = None, scaled: int | None = None, seed: int = 42, device: int = 0) -> tuple:
    """ksp_sketch_host_abund: sketch_host with every key's abundance, counted on the device -> (keys, abund, offsets, stats)."""
    return _sketch_host(lib().ksp_sketch_host_abund, (), True, seq, src_offsets, ksize, max_hash, scaled, seed, device)


def sketch_device_abund(d_seq_ptr: int, n_bytes: int, src_offsets, ksize: int, max_hash: int, d_out_keys_ptr: int, d_out_abund_ptr: int, capacity: int, seed: int = 42,
                        device: int = 0) -> tuple:
    """ksp_sketch_device_abund: sketch_device with d_out_abund (DEVICE, room for `capacity`) beside the keys -> (rc, offsets, stats)."""
    return _sketch_device(lib().ksp_sketch_device_abund, (), int(d_out_abund_ptr or 0), d_seq_ptr, n_bytes, src_offsets, ksize, max_hash, d_out_keys_ptr, capacity, seed, device)


def sketch_host(seq, src_offsets, ksize: int, max_hash: int | None = None, scaled: int | None = None, seed: int = 42, device: int = 0) -> tuple:
    """ksp_sketch_host: host bytes and source offsets -> (keys, offsets, stats) of the sources' sketches, made on the device."""
    return _sketch_host(lib().ksp_sketch_host, (), None, seq, src_offsets, ksize, max_hash, scaled, seed, device)


def sketch_device(d_seq_ptr: int, n_bytes: int, src_offsets, ksize: int, max_hash: int, d_out_keys_ptr: int, capacity: int, seed: int = 42,
                  device: int = 0) -> tuple:
    """ksp_sketch_device: bytes and keys in DEVICE memory, offsets on the host (d_out_keys 0 / capacity 0: the size query).
    -> (rc, offsets, stats): rc is KSP_OK or KSP_E_OVERFLOW (stats["needed"] is then the required capacity); anything else raises."""
    return _sketch_device(lib().ksp_sketch_device, (), None, d_seq_ptr, n_bytes, src_offsets, ksize, max_hash, d_out_keys_ptr, capacity, seed, device)


def fastx_read(path: str) -> dict:
    """A FASTA / FASTQ file, plain or gzip (ksp_fastx_info + ksp_fastx_load; host only): seq (every record's bases followed by one
    newline), rec_offsets, names (every header's first word), fastq."""
    info = np.zeros(4, dtype=np.uint64)
    _check(lib().ksp_fastx_info(os.fsencode(path), info.ctypes.data))
    R, B, T = int(info[0]), int(info[1]), int(info[2])
    seq, text = np.zeros(B + 1, dtype=np.uint8), np.zeros(T + 1, dtype=np.uint8)
    rec_off, name_off = np.zeros(R + 1, dtype=np.uint64), np.zeros(R + 1, dtype=np.uint64)
    _check(lib().ksp_fastx_load(os.fsencode(path), seq.ctypes.data, rec_off.ctypes.data, name_off.ctypes.data, text.ctypes.data))
    blob = text[:T].tobytes()
    return {"seq": seq[:B].tobytes(), "rec_offsets": rec_off, "names": [os.fsdecode(blob[int(name_off[r]):int(name_off[r + 1])]) for r in range(R)],
            "fastq": bool(info[3])}


def _moltype(moltype) -> int:
    """A molecule type by number or by name ("dna", "protein", "dayhoff", "hp"); an unknown number is passed on and refused by the library."""
    if isinstance(moltype, str):
        if moltype.lower() not in _MOLTYPES:
            raise ValueError("moltype is dna, protein, dayhoff or hp")
        return _MOLTYPES[moltype.lower()]
    return int(moltype)


def sketch_text_hash(text, moltype, seed: int = 42) -> tuple:
    """(hash, valid) of the one k-mer the residue bytes spell for a protein, dayhoff or hp moltype (host only); valid is False, and
    hash 0, when a byte is neither a letter nor '*'."""
    text = text.encode() if isinstance(text, str) else bytes(text)
    h, v = ctypes.c_uint64(0), ctypes.c_int(0)
    _check(lib().ksp_sketch_text_hash(text, len(text), _moltype(moltype), int(seed), ctypes.byref(h), ctypes.byref(v)))
    return h.value, bool(v.value)


def sketch_cpu_mol(seq, src_offsets, ksize: int, moltype, translate: bool = False, max_hash: int | None = None, scaled: int | None = None, seed: int = 42,
                   abund: bool = False) -> tuple:
    """ksp_sketch_cpu_mol, the plain host loop for a molecule type: residue bytes, or with translate DNA read in six frames ->
    (keys, offsets), with abund (keys, abund, offsets).  No GPU."""
    return _sketch_cpu(lib().ksp_sketch_cpu_mol, (_moltype(moltype), SKETCH_TRANSLATE if translate else 0), bool(abund), seq, src_offsets, ksize, max_hash, scaled, seed)


def sketch_host_mol(seq, src_offsets, ksize: int, moltype, translate: bool = False, max_hash: int | None = None, scaled: int | None = None, seed: int = 42,
                    abund: bool = False, device: int = 0) -> tuple:
    """ksp_sketch_host_mol: sketch_cpu_mol's result made on the device -> (keys, offsets, stats), with abund (keys, abund, offsets, stats)."""
    return _sketch_host(lib().ksp_sketch_host_mol, (_moltype(moltype), SKETCH_TRANSLATE if translate else 0), bool(abund), seq, src_offsets, ksize, max_hash, scaled, seed,
                        device)


def sketch_device_mol(d_seq_ptr: int, n_bytes: int, src_offsets, ksize: int, moltype, translate: bool, max_hash: int, d_out_keys_ptr: int, d_out_abund_ptr: int,
                      capacity: int, seed: int = 42, device: int = 0) -> tuple:
    """ksp_sketch_device_mol: bytes, keys and (d_out_abund_ptr 0: no) counts in DEVICE memory, offsets on the host -> (rc, offsets,
    stats): rc is KSP_OK or KSP_E_OVERFLOW (stats["needed"] is then the required capacity); anything else raises."""
    return _sketch_device(lib().ksp_sketch_device_mol, (_moltype(moltype), SKETCH_TRANSLATE if translate else 0), int(d_out_abund_ptr or 0), d_seq_ptr, n_bytes, src_offsets,
                          ksize, max_hash, d_out_keys_ptr, capacity, seed, device)


def sketch_files(input_path: str, kSize: int, scaled: int, out_dir: str, user_threads: int = 1, per_record: bool = False, seed: int | None = None,
                 abund: bool = False, moltype=MOL_DNA, translate: bool = False) -> None:
    """FASTA / FASTQ files -> one sourmash-compatible .sig file per source in out_dir (kspider_sketch).  input_path: a directory
    (each file a source) or one file (per_record: each record a source); abund: every hash's abundance beside it ("abundances").
    moltype protein, dayhoff or hp: kSize is the residue k, the input protein (.faa .fa .fasta) or, with translate, DNA read in six
    frames; the files say "ksize": 3 * kSize.  KSPIDER_SKETCH=host in the environment: no GPU."""
    flags = (SKETCH_PER_RECORD if per_record else 0) | (0 if seed is None else SKETCH_SEED | (int(seed) << 32)) | (SKETCH_ABUND if abund else 0)
    flags |= {MOL_DNA: 0, MOL_PROTEIN: SKETCH_PROTEIN, MOL_DAYHOFF: SKETCH_DAYHOFF, MOL_HP: SKETCH_HP}[_moltype(moltype)] | (SKETCH_TRANSLATE if translate else 0)
    _check(lib().kspider_sketch(os.fsencode(input_path), int(kSize), int(scaled), os.fsencode(out_dir), int(user_threads), flags))


_CLASSIFY_ARRAYS = ("kept_windows", "matched", "n_refs_hit", "best_ref", "best_hits", "second_hits")


def _classify_results(n_records, call):
    """The results of a classify call: call(rows, n_rows, the six arrays' addresses, stats) -> (rows, {array name: uint32[n_records]}, stats)."""
    arrays = {name: np.zeros(max(int(n_records), 1), dtype=np.uint32) for name in _CLASSIFY_ARRAYS}
    out = ctypes.c_void_p()
    nr = ctypes.c_uint64(0)
    st = ClassifyStats()
    _check(call(ctypes.byref(out), ctypes.byref(nr), *[arrays[name].ctypes.data for name in _CLASSIFY_ARRAYS], ctypes.byref(st)))
    rows = _take(out, nr.value, CLASSIFY_ROW_DTYPE)
    return rows, {name: a[:int(n_records)] for name, a in arrays.items()}, st.as_dict()


def _classify_one_shot(entry, lead, seq, rec_offsets, ksize, ref_keys, ref_offsets, min_hits, max_hash, scaled, seed):
    buf, off, mh = _sketch_input(seq, rec_offsets, max_hash, scaled)
    rk, ro = _u64(ref_keys), _u64(ref_offsets)
    n_rec = max(off.size - 1, 0)
    return _classify_results(n_rec, lambda *res: entry(*lead, _ptr(buf), buf.size, _ptr(off), n_rec, int(ksize), mh, int(seed), _ptr(rk), _ptr(ro), _n_sketches(ro),
                                                       int(min_hits), *res))


def classify_cpu(seq, rec_offsets, ksize: int, ref_keys, ref_offsets, min_hits: int = 1, max_hash: int | None = None, scaled: int | None = None, seed: int = 42) -> tuple:
    """ksp_classify_cpu, the plain host loop: the records of a byte stream against references (strictly ascending runs of hashes)
    -> (rows ordered by (record, reference), {kept_windows, matched, n_refs_hit, best_ref, best_hits, second_hits}, stats).  No GPU."""
    return _classify_one_shot(lib().ksp_classify_cpu, (), seq, rec_offsets, ksize, ref_keys, ref_offsets, min_hits, max_hash, scaled, seed)


def classify_host(seq, rec_offsets, ksize: int, ref_keys, ref_offsets, min_hits: int = 1, max_hash: int | None = None, scaled: int | None = None, seed: int = 42,
                  device: int = 0) -> tuple:
    """ksp_classify_host: classify_cpu's result made on the device, in one batch."""
    return _classify_one_shot(lib().ksp_classify_host, (int(device),), seq, rec_offsets, ksize, ref_keys, ref_offsets, min_hits, max_hash, scaled, seed)


class ClassifySession:
    """ksp_classify_open / _add / _finish / _close: the table once, a batch of segments with their record ids per add(), the
    results once.  close() may be called at any time; the object is also a context manager."""

    def __init__(self, ksize: int, ref_keys, ref_offsets, max_hash: int | None = None, scaled: int | None = None, seed: int = 42, device: int = 0):
        if (max_hash is None) == (scaled is None):
            raise ValueError("give max_hash or scaled")
        rk, ro = _u64(ref_keys), _u64(ref_offsets)
        self._h = ctypes.c_void_p()
        _check(lib().ksp_classify_open(int(device), int(ksize), sketch_max_hash(scaled) if max_hash is None else int(max_hash), int(seed), _ptr(rk), _ptr(ro),
                                       _n_sketches(ro), ctypes.byref(self._h)))

    def add(self, seq, seg_offsets, seg_records) -> None:
        buf = np.frombuffer(bytes(seq), dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(seg_offsets, dtype=np.uint64)
        rec = None if seg_records is None else np.ascontiguousarray(seg_records, dtype=np.uint32)
        _check(lib().ksp_classify_add(self._h, _ptr(buf), buf.size, _ptr(off), _ptr(rec), max(off.size - 1, 0)))

    def finish(self, n_records: int, min_hits: int = 1) -> tuple:
        return _classify_results(n_records, lambda *res: lib().ksp_classify_finish(self._h, int(n_records), int(min_hits), *res))

    def close(self) -> None:
        if self._h:
            lib().ksp_classify_close(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def classify_files(input_path: str, kSize: int, scaled: int, db: str, out_prefix: str, user_threads: int = 1, min_hits: int = 1) -> None:
    """Every read or contig of FASTA / FASTQ input against a sketch database (kspider_classify): input_path is one file or a
    directory, db a directory of .sig files or a pack file; writes OUT_kSpider_classify.tsv (one row per record) and
    OUT_kSpider_classify_hits.tsv (one row per record and reference with at least min_hits shared hashes).
    KSPIDER_CLASSIFY=host in the environment: no GPU."""
    _check(lib().kspider_classify(os.fsencode(input_path), int(kSize), int(scaled), os.fsencode(db), os.fsencode(out_prefix) if out_prefix else None, int(user_threads),
                                  int(min_hits)))


def cluster_from_tree(index_prefix: str, dist_type: str = "max_cont", cutoff: float = 0.0) -> None:
    """`kSpider cluster -i PREFIX -d DIST -c CUTOFF` from PREFIX_kSpider_tree_<DIST>.tsv alone (host only): the same file, byte for byte."""
    _check(lib().kspider_cluster_from_tree(os.fsencode(index_prefix), dist_type.encode() if dist_type is not None else None, float(cutoff)))


def estimate_ani(index_prefix: str, user_threads: int, scale: int) -> None:
    """`kSpider pairwise -i PREFIX --estimate-ani -s SCALE` (ks_pairwise.py:29-84) over the files already there: writes
    PREFIX_kSpider_pairwise.ani_col.tsv.  Host only; k is the first line of PREFIX.extra."""
    _check(lib().kspider_estimate_ani(os.fsencode(index_prefix), int(user_threads), int(scale)))


def pairwise_ani(index_prefix: str, user_threads: int, scale: int, cutoff: float | None = None) -> None:
    """`kSpider pairwise` and `pairwise --estimate-ani` in one device pass (both TSVs as kspider_pairwise writes them, plus
    the ANI column); with a cutoff also `kSpider cluster -d ani -c CUTOFF`, the components taken from the edges in HBM."""
    L = lib()
    if cutoff is None:
        _check(L.kspider_pairwise_ani(os.fsencode(index_prefix), int(user_threads), int(scale)))
    else:
        _check(L.kspider_pairwise_ani_and_cluster(os.fsencode(index_prefix), int(user_threads), int(scale), float(cutoff)))


def edges_ani(d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, ksize: int, d_ani_ptr: int, device: int = 0) -> None:
    """d_ani[e] = average ANI of the ksp_edge record e (all DEVICE pointers); KspError on a NaN containment."""
    _check(lib().ksp_edges_ani(device, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(ksize), d_ani_ptr or None))


def components_edges_ani(n_nodes: int, d_edges_ptr: int, n_edges: int, d_kmer_counts_ptr: int, ksize: int, cutoff: float,
                         device: int = 0) -> np.ndarray:
    """components_edges with the ANI column as the distance: an edge counts when ani * 100 is not below cutoff * 100."""
    out = np.empty(max(1, n_nodes), dtype=np.uint32)
    _check(lib().ksp_components_edges_ani(device, n_nodes, d_edges_ptr or None, n_edges, d_kmer_counts_ptr or None, int(ksize),
                                          float(cutoff), out.ctypes.data))
    return out[:n_nodes]


def ani_values(min_c: np.ndarray, max_c: np.ndarray, ksize: int, via_table: bool) -> tuple:
    """(rc, values): the ANI of rows with these containment floats, by the text definition or the device's table path."""
    mn = np.ascontiguousarray(min_c, dtype=np.float32)
    mx = np.ascontiguousarray(max_c, dtype=np.float32)
    out = np.empty(mn.size, dtype=np.float64)
    rc = lib().ksp_ani_values(mn.ctypes.data, mx.ctypes.data, mn.size, int(ksize), int(bool(via_table)), out.ctypes.data)
    return rc, out


def format_ani(v: float) -> str:
    buf = ctypes.create_string_buffer(32)
    n = lib().ksp_format_ani(float(v), buf)
    return buf.raw[:n].decode()


def export(index_prefix: str, dist_type: str = "max_cont", newick: bool = False, out_prefix: str | None = None) -> None:
    """`kSpider export -i PREFIX -d DIST [--newick] [-o OUT]` (ks_export.py): the named pairwise TSV, the N x N distance
    matrix and, with newick, the single-linkage tree computed on the GPU.  out_prefix None: the reference's names
    (kSpider_<basename>_...) in the current directory."""
    _check(lib().kspider_export(os.fsencode(index_prefix), dist_type.encode(), int(bool(newick)),
                                os.fsencode(out_prefix) if out_prefix else None))


def single_linkage_rows(d_rows_ptr: int, n: int, device: int = 0) -> np.ndarray:
    """scipy.cluster.hierarchy.linkage(rows, 'single') of the n x n row-major float64 matrix at DEVICE pointer d_rows_ptr,
    bit for bit: an (n - 1) x 4 float64 array."""
    Z = np.empty((max(int(n) - 1, 0), 4), dtype=np.float64)
    _check(lib().ksp_single_linkage_rows(int(device), int(n), d_rows_ptr or None, Z.ctypes.data if Z.size else None))
    return Z


def single_linkage_prim(d_rows_ptr: int, n: int, device: int = 0) -> np.ndarray:
    """Prim's (x, y, height, m) rows of single_linkage_rows in the order they are found (before the sort and relabel):
    x the node merged last, m the merged node nearest to y (height = distance(m, y))."""
    P = np.empty((max(int(n) - 1, 0), 4), dtype=np.float64)
    _check(lib().ksp_single_linkage_prim(int(device), int(n), d_rows_ptr or None, P.ctypes.data if P.size else None))
    return P


def row_distances(d_rows_ptr: int, n: int, device: int = 0) -> np.ndarray:
    """(tests) The n x n float64 matrix of distances between the rows of the n x n row-major float64 matrix at DEVICE
    pointer d_rows_ptr, as the device computes it for the two linkage entries above: scipy's pdist in square form."""
    S = np.empty((max(int(n), 0), max(int(n), 0)), dtype=np.float64)
    _check(lib().ksp_row_distances(int(device), int(n), d_rows_ptr or None, S.ctypes.data if S.size else None))
    return S


def csv_float(text: str) -> float:
    """The value pandas' read_csv makes of one cell's text (its default, not correctly rounded, parser)."""
    out = ctypes.c_double()
    _check(lib().ksp_csv_float(text.encode(), ctypes.byref(out)))
    return out.value


def components(n_nodes: int, a: np.ndarray, b: np.ndarray, device: int = 0) -> np.ndarray:
    """Connected components of an undirected edge list on the GPU: label[v] = smallest node of v's component."""
    a = np.ascontiguousarray(a, dtype=np.uint32)
    b = np.ascontiguousarray(b, dtype=np.uint32)
    out = np.empty(n_nodes, dtype=np.uint32)
    _check(lib().ksp_components(device, n_nodes, a.ctypes.data, b.ctypes.data, a.size, out.ctypes.data))
    return out


def index_info(index_prefix: str) -> dict:
    out = (ctypes.c_uint64 * 6)()
    _check(lib().ksp_index_info(os.fsencode(index_prefix), out))
    return dict(colors=out[0], groups=out[1], color_counts=out[2], sources=out[3], kwidth=out[4], trailer=bool(out[5]))


def format_float(v: float) -> str:
    buf = ctypes.create_string_buffer(32)
    n = lib().ksp_format_float(ctypes.c_float(v), buf)
    return buf.raw[:n].decode()


class Engine:
    """Device-resident engine: build_blocks() once per sketch set, join() per tile range."""

    def __init__(self, device: int = 0):
        self.device = device
        self._h = ctypes.c_void_p()
        _check(lib().ksp_engine_create(device, ctypes.byref(self._h)))

    def close(self):
        if self._h:
            lib().ksp_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def build_blocks(self, d_keys_ptr: int, h_offsets: np.ndarray, d_weights_ptr: int = 0, key_bits: int = 0,
                     stream: int = 0):
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        self._off = h_offsets
        _check(lib().ksp_engine_build_blocks(self._h, d_keys_ptr or None, d_weights_ptr or None,
                                             h_offsets.ctypes.data, h_offsets.size - 1, key_bits, stream or None))

    def step_launch(self, d_keys_ptr: int, h_offsets: np.ndarray, part: int, nparts: int, d_edges_ptr: int, capacity: int,
                    stream: int = 0, d_weights_ptr: int = 0, key_bits: int = 0):
        """build_blocks + this rank's tile range + join_launch on it in one call (include/kspider_amd.h).  Returns
        (t0, t1, bound, launched, prev_count); launched False: the bound does not fit `capacity`, call join_launch(t0, t1, ...);
        prev_count: the count of the join that was pending on this engine (None: there was none).
        If that join failed (KSP_E_OVERFLOW: its buffer was too small), PrevJoinError carries its status and, in .step, this
        call's return value: the new step was built (and launched) all the same."""
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        self._off = h_offsets
        L = lib()
        L.ksp_engine_step_launch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        rng = (ctypes.c_uint64 * 2)()
        bound = ctypes.c_uint64(0)
        prev = ctypes.c_uint64(0)
        prev_rc = ctypes.c_int(0)
        prev_ms = ctypes.c_float(0)
        had = bool(getattr(self, "_join_in_flight", False))
        rc = L.ksp_engine_step_launch(self._h, d_keys_ptr or None, d_weights_ptr or None, h_offsets.ctypes.data, h_offsets.size - 1,
                                      key_bits, part, nparts, d_edges_ptr or None, capacity, rng, ctypes.byref(bound), ctypes.byref(prev),
                                      ctypes.byref(prev_rc), ctypes.byref(prev_ms), stream or None)
        # the engine's state first: KSP_OK / KSP_E_OVERFLOW built this step (and collected the previous join), KSP_OK launched
        # its join; KSP_E_ARG / KSP_E_LIMIT refused the call before anything changed (a pending join stays pending)
        if rc in (KSP_OK, KSP_E_OVERFLOW):
            self._join_in_flight = rc == KSP_OK
        elif rc not in (KSP_E_ARG, KSP_E_LIMIT):
            self._join_in_flight = False
        self.prev_ms_join = float(prev_ms.value)
        if rc not in (KSP_OK, KSP_E_OVERFLOW):
            _check(rc)
        step = (int(rng[0]), int(rng[1]), int(bound.value), rc == KSP_OK, (int(prev.value) if had else None))
        if prev_rc.value != KSP_OK:
            raise PrevJoinError(prev_rc.value, f"the previous step's join failed with status {prev_rc.value} "
                                "(KSP_E_OVERFLOW: its edge buffer was too small); this step went ahead: see .step", step)
        return step

    def build_postings(self, h_key_off: np.ndarray, d_sources_ptr: int, d_key_weights_ptr: int, n_sources: int,
                       stream: int = 0):
        """Stage 1 from an inverted index: key k is held by d_sources[key_off[k]:key_off[k+1]] (device uint32)."""
        h_key_off = np.ascontiguousarray(h_key_off, dtype=np.uint64)
        self._off = h_key_off
        _check(lib().ksp_engine_build_postings(self._h, h_key_off.ctypes.data, d_sources_ptr or None,
                                               d_key_weights_ptr or None, h_key_off.size - 1, n_sources, stream or None))

    def build_postings_slice(self, h_key_off: np.ndarray, d_sources_ptr: int, d_key_weights_ptr: int, n_sources: int,
                             stream: int = 0):
        """One slice of an inverted index (any subset of its keys, every key with all its holders; h_key_off from 0), up
        to the source labels: then slice_labels (MIN over the slices), slice_bounds (SUM over the slices),
        slice_set_bounds, slice_finish, slice_export, assemble.  Without set_bounds the slice takes 32-bit pair counters
        everywhere: its own share of a source's keys / weights is no bound for the assembled lists."""
        h_key_off = np.ascontiguousarray(h_key_off, dtype=np.uint64)
        self._off = h_key_off
        _check(lib().ksp_engine_build_postings_slice(self._h, h_key_off.ctypes.data, d_sources_ptr or None,
                                                     d_key_weights_ptr or None, h_key_off.size - 1, n_sources,
                                                     stream or None))

    # ---- key-range sharded stage 1 (multi-GPU) ------------------------------------------------
    def build_slice(self, d_keys_ptr: int, h_offsets: np.ndarray, part: int, nparts: int, d_weights_ptr: int = 0,
                    key_bits: int = 0, stream: int = 0):
        h_offsets = np.ascontiguousarray(h_offsets, dtype=np.uint64)
        self._off = h_offsets
        _check(lib().ksp_engine_build_slice(self._h, d_keys_ptr or None, d_weights_ptr or None,
                                            h_offsets.ctypes.data, h_offsets.size - 1, key_bits, part, nparts,
                                            stream or None))

    def slice_labels(self, d_labels: int, stream: int = 0):
        """Copy the slice's source labels (n_sources uint32) into a device buffer."""
        _check(lib().ksp_engine_slice_labels(self._h, d_labels, stream or None))

    def slice_bounds(self, d_bounds: int, stream: int = 0):
        """Copy the slice's per-source counter bounds (n_sources uint32: keys / weight sum) into a device buffer."""
        _check(lib().ksp_engine_slice_bounds(self._h, d_bounds, stream or None))

    def slice_set_bounds(self, d_bounds: int, stream: int = 0):
        """The bounds summed over the slices of an inverted index, before slice_finish (include/kspider_amd.h)."""
        _check(lib().ksp_engine_slice_set_bounds(self._h, d_bounds, stream or None))

    def slice_finish(self, d_labels: int = 0, stream: int = 0):
        """Second half of a slice build, in the source order given by the combined labels."""
        _check(lib().ksp_engine_slice_finish(self._h, d_labels or None, stream or None))

    def slice_sizes(self) -> np.ndarray:
        out = (ctypes.c_uint64 * 4)()
        _check(lib().ksp_engine_slice_sizes(self._h, out))
        return np.array(list(out), dtype=np.uint64)

    def slice_export(self, d_brk: int, d_info: int, d_bw: int, d_blk_raw: int, d_blk_pos: int, d_big: int,
                     stream: int = 0):
        _check(lib().ksp_engine_slice_export(self._h, d_brk or None, d_info or None, d_bw or None, d_blk_raw or None,
                                             d_blk_pos or None, d_big or None, stream or None))

    def assemble(self, h_sizes: np.ndarray, d_brk_all: int, d_info_all: int, d_bw_all: int, lstride: int,
                 d_blk_raw_all: int, d_blk_pos_all: int, d_big_all: int, bigstride: int, stream: int = 0):
        h_sizes = np.ascontiguousarray(h_sizes, dtype=np.uint64)
        nparts = h_sizes.size // 4
        _check(lib().ksp_engine_assemble(self._h, nparts, h_sizes.ctypes.data, d_brk_all or None, d_info_all or None,
                                         d_bw_all or None, lstride, d_blk_raw_all or None, d_blk_pos_all or None,
                                         d_big_all or None, bigstride, stream or None))

    @property
    def num_tiles(self) -> int:
        return lib().ksp_engine_num_tiles(self._h)

    def tile_pairs(self, t0: int, t1: int) -> int:
        return lib().ksp_engine_tile_pairs(self._h, t0, t1)

    def balanced_cuts(self, nparts: int) -> list:
        """Tile ranges of equal estimated work: rank p joins tiles [cuts[p], cuts[p + 1])."""
        out = (ctypes.c_uint64 * (nparts + 1))()
        _check(lib().ksp_engine_balanced_cuts(self._h, nparts, out))
        return [int(x) for x in out]

    def source_order(self, n_sources: int) -> np.ndarray:
        """(diagnostics) engine index (block x 128 + slot) of every source of the last build."""
        L = lib()
        L.ksp_engine_source_order.restype = ctypes.c_int
        L.ksp_engine_source_order.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        out = np.zeros(max(1, n_sources), dtype=np.uint32)
        _check(L.ksp_engine_source_order(self._h, out.ctypes.data_as(ctypes.c_void_p)))
        return out[:n_sources]

    def edge_bound(self, t0: int, t1: int) -> int:
        """Upper bound on the edges of tiles [t0, t1): source pairs of the tiles that share a key."""
        return lib().ksp_engine_edge_bound(self._h, t0, t1)

    def join_launch(self, t0: int, t1: int, d_edges_ptr: int, capacity: int, stream: int = 0) -> None:
        """Queue the join on `stream` and return; join_wait() collects the count (see include/kspider_amd.h)."""
        _check(lib().ksp_engine_join_launch(self._h, t0, t1, d_edges_ptr or None, capacity, ctypes.c_void_p(stream)))
        self._join_in_flight = True

    def join_wait(self) -> int:
        cnt = ctypes.c_uint64(0)
        self._join_in_flight = False
        _check(lib().ksp_engine_join_wait(self._h, ctypes.byref(cnt)))
        return int(cnt.value)

    def join_to_host(self, t0: int, t1: int, h_edges_ptr: int, capacity: int, stream: int = 0) -> int:
        """Join tiles [t0, t1) piece by piece, every piece copied to (pinned) host memory under the join of the next."""
        cnt = ctypes.c_uint64(0)
        L = lib()
        L.ksp_engine_join_to_host.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                              ctypes.c_void_p, ctypes.c_void_p]
        rc = L.ksp_engine_join_to_host(self._h, t0, t1, h_edges_ptr or None, capacity, ctypes.byref(cnt), stream or None)
        if rc == KSP_E_OVERFLOW:
            err = KspError(rc, L.ksp_last_error().decode())
            err.count = int(cnt.value)
            raise err
        _check(rc)
        return int(cnt.value)

    def join(self, t0: int, t1: int, d_edges_ptr: int, capacity: int, stream: int = 0) -> int:
        cnt = ctypes.c_uint64(0)
        _check(lib().ksp_engine_join(self._h, t0, t1, d_edges_ptr or None, capacity, ctypes.byref(cnt),
                                     stream or None))
        return cnt.value

    def set_profiling(self, on: bool = True):
        """Record one HIP event per phase start of every later build (see phase_times)."""
        _check(lib().ksp_engine_set_profiling(self._h, int(bool(on))))

    def phase_times(self) -> list:
        """[(phase name, ms)] of the last build made with profiling on."""
        names = (ctypes.c_char_p * 24)()
        ms = (ctypes.c_float * 24)()
        n = lib().ksp_engine_phase_times(self._h, names, ms, 24)
        return [(names[i].decode(), float(ms[i])) for i in range(n)]

    def lists_path(self) -> int:
        """How the last build made its block lists: LISTS_NONE / KEYED / COMPACTED / SORTED / FUSED."""
        v = ctypes.c_int(0)
        _check(lib().ksp_engine_lists_path(self._h, ctypes.byref(v)))
        return int(v.value)

    def stats(self) -> dict:
        st = Stats()
        _check(lib().ksp_engine_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def ms_join(self) -> float:
        """HIP-event time of the last collected join (one field of the stats, without building the dict)."""
        st = Stats()
        _check(lib().ksp_engine_get_stats(self._h, ctypes.byref(st)))
        return float(st.ms_join)


class DeviceBuffer:
    """hipMalloc'ed buffer through the C ABI (tests use it instead of torch)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.ptr = ctypes.c_void_p()
        self.nbytes = int(nbytes)
        _check(lib().ksp_device_malloc(device, self.nbytes, ctypes.byref(self.ptr)))

    @classmethod
    def from_numpy(cls, a: np.ndarray, device: int = 0):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes, device)
        _check(lib().ksp_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes))
        return b

    def to_numpy(self, dtype, count: int) -> np.ndarray:
        out = np.empty(count, dtype=dtype)
        _check(lib().ksp_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ksp_device_free(self.ptr)
            self.ptr = ctypes.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
