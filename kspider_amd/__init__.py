"""kspider_amd — MI355X-native pairwise containment engine behind kSpider's pairwise() surface.

Host-side mirror of the reference interface for this one path:
  kspider_amd.pairwise(index_prefix, user_threads)   == kSpider_internal.pairwise (kSpider_internal.i:11)
  kspider_amd.cluster(index_prefix, dist_type, cutoff)  == `kSpider cluster` (ks_clustering.py:150-163), components on the GPU
  kspider_amd.estimate_ani(index_prefix, threads, scale) == `kSpider pairwise --estimate-ani` (ks_pairwise.py:29-84), host only
  kspider_amd.pairwise_ani(index_prefix, threads, scale[, cutoff])  pairwise + ANI column (+ `cluster -d ani`) in one pass
  kspider_amd.export(index_prefix, dist_type, newick, out_prefix)  == `kSpider export` (ks_export.py), linkage on the GPU
  kspider_amd.pairwise_cut(index_prefix, threads, dist_type, cutoff)  pairwise with a minimum containment, cut on the GPU
  kspider_amd.cluster_sweep(index_prefix, dist_type, cutoffs)  `kSpider cluster` at a list of cut-offs in one device pass
  kspider_amd.tree(index_prefix, dist_type, newick)  the single-linkage tree of the pairwise TSV (maximum spanning forest on the GPU)
  kspider_amd.cluster_from_tree(index_prefix, dist_type, cutoff)  `kSpider cluster` at any cut-off from the tree file alone
  kspider_amd.query(db, queries, kSize, out_prefix, threads, mode)  new sketches against a database, without the N x N join
  kspider_amd.gather(db, queries, kSize, out_prefix, threads, min_hashes, max_matches)  what each query is made of: greedy set cover
  kspider_amd.gather_abund(db, queries, kSize, out_prefix, threads, min_hashes, max_matches)  the same for signatures with abundances: weighted columns
  kspider_amd.compare(samples, kSize, out_prefix, threads, against, matrix)  counted sketches against each other: cosine, angular similarity, weighted containment
  kspider_amd.pack(sketch_dir, kSize, out_path, threads)  a directory of sketches as one database file
  kspider_amd.sketch_files(input, kSize, scaled, out_dir, threads)  FASTA / FASTQ in, sourmash-compatible .sig files out, hashed on the GPU
      (moltype="protein" | "dayhoff" | "hp", translate=True: protein sketches of proteomes, or of genomes read in six frames)
  kspider_amd.engine                                   ctypes binding of include/kspider_amd.h
  kspider_amd.dist                                     tile sharding + edge gather for one-process-per-GPU runs
  kspider_amd.synth                                    synthetic sketch sets shaped like BASELINE.json's configs
The compute lives in kspider_amd/lib/libkspider_amd.so (hand-written HIP, gfx950); nothing here
falls back to the CPU.
"""
from .engine import cluster, estimate_ani, export, pairwise, pairwise_ani, pairwise_bins, pairwise_sigs  # noqa: F401
from .engine import cluster_sweep, pairwise_and_cluster_sweep  # noqa: F401
from .engine import UPGMA_CHUNK_EDGES, UPGMA_ROW_DTYPE, UPGMA_TAIL_PAIRS, cluster_from_upgma, edges_upgma, pairwise_and_upgma, upgma, upgma_before, upgma_valued  # noqa: F401
from .engine import TREE_CHUNK_EDGES, cluster_from_tree, edges_forest, forest_ranked, pairwise_and_tree, tree  # noqa: F401
from .engine import single_linkage_rows  # noqa: F401
from .engine import CUT_CHUNK_EDGES, edges_cut, pairwise_cut, pairwise_host_cut  # noqa: F401
from .engine import QUERY_CROSS, QUERY_CROSS_AND_SELF, pack, query  # noqa: F401
from .engine import GATHER_ROW_DTYPE, GatherStats, gather, gather_device, gather_host  # noqa: F401
from .engine import GATHER_WROW_DTYPE, GatherWRow, gather_abund, gather_abund_device, gather_abund_host, sig_read  # noqa: F401
from .engine import WEDGE_DTYPE, CompareStats, Wedge, compare, compare_device, compare_host, compare_values  # noqa: F401
from .engine import SketchStats, sketch_cpu, sketch_device, sketch_files, sketch_host, sketch_max_hash  # noqa: F401
from .engine import sketch_cpu_abund, sketch_device_abund, sketch_host_abund  # noqa: F401
from .engine import sketch_cpu_mol, sketch_device_mol, sketch_host_mol, sketch_text_hash  # noqa: F401

__all__ = ["pairwise", "pairwise_sigs", "pairwise_bins", "cluster", "estimate_ani", "pairwise_ani", "export",
           "query", "pack", "QUERY_CROSS", "QUERY_CROSS_AND_SELF",
           "gather", "gather_host", "gather_device", "GatherStats", "GATHER_ROW_DTYPE",
           "gather_abund", "gather_abund_host", "gather_abund_device", "GatherWRow", "GATHER_WROW_DTYPE", "sig_read",
           "compare", "compare_host", "compare_device", "compare_values", "CompareStats", "Wedge", "WEDGE_DTYPE",
           "sketch_cpu_abund", "sketch_host_abund", "sketch_device_abund",
           "sketch_cpu_mol", "sketch_host_mol", "sketch_device_mol", "sketch_text_hash",
           "sketch_files", "sketch_host", "sketch_device", "sketch_cpu", "sketch_max_hash", "SketchStats",
           "single_linkage_rows", "pairwise_cut", "pairwise_host_cut", "edges_cut", "CUT_CHUNK_EDGES",
           "cluster_sweep", "pairwise_and_cluster_sweep",
           "tree", "pairwise_and_tree", "cluster_from_tree", "edges_forest", "forest_ranked", "TREE_CHUNK_EDGES"]
