"""The cut-off ladder restated (tests only): per cut-off, a union-find over the edges `kSpider cluster` keeps at that cut-off
(cut_restate.keep on the text of the edge's own column value); an edge's level is the number of the given cut-offs that keep
it.  Nothing here calls the code under test; a float becomes text through engine.format_float, which existing tests pin."""
import numpy as np

import cut_restate as cr
from kspider_amd import engine


def union_find(n: int, a, b) -> np.ndarray:
    """label[v] = smallest node of v's component."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n)], dtype=np.uint32)


def column_texts(edges: np.ndarray, kmer_counts: np.ndarray, col: int) -> list:
    """The text of every edge's column value, as the pairwise TSV prints it (what cut_restate.edge_mask tests, made once)."""
    return [engine.format_float(v) for v in cr.column_values(edges, np.asarray(kmer_counts), col).tolist()]


def masks(texts: list, cutoffs) -> np.ndarray:
    """[K, n_edges] bool: row i = the edges cut-off i keeps (cut_restate.keep, asked once per distinct text and cut-off)."""
    distinct = sorted(set(texts))
    place = {t: i for i, t in enumerate(distinct)}
    table = np.array([[cr.keep(t, float(c)) for t in distinct] for c in cutoffs], dtype=bool).reshape(len(cutoffs), len(distinct))
    return table[:, np.array([place[t] for t in texts], dtype=np.int64)]


def levels(texts: list, cutoffs) -> np.ndarray:
    """Per edge, the number of the given cut-offs that keep it."""
    return masks(texts, cutoffs).sum(axis=0).astype(np.uint8)


def components(n_nodes: int, edges: np.ndarray, kmer_counts: np.ndarray, col: int, cutoff: float) -> np.ndarray:
    """The labels at one cut-off, through cut_restate.edge_mask."""
    m = cr.edge_mask(edges, kmer_counts, col, cutoff)
    return union_find(n_nodes, edges["source_1"][m], edges["source_2"][m])


def ladder(n_nodes: int, edges: np.ndarray, texts: list, cutoffs) -> tuple:
    """(labels[K, n_nodes], kept[K]) in the order of the given cut-offs."""
    mk = masks(texts, cutoffs)
    labels = np.array([union_find(n_nodes, edges["source_1"][m], edges["source_2"][m]) for m in mk], dtype=np.uint32).reshape(len(cutoffs), n_nodes)
    return labels, mk.sum(axis=1).astype(np.uint64)


def strictness_ranks(texts_probe: list, cutoffs) -> np.ndarray:
    """rank[i] of cut-off i: the cut-offs sorted by how many of the probe texts they keep, most first (ties in any order)."""
    kept = masks(texts_probe, cutoffs).sum(axis=1)
    order = np.argsort(-kept, kind="stable")
    rank = np.empty(len(cutoffs), dtype=np.int64)
    rank[order] = np.arange(len(cutoffs))
    return rank


def per_rank_components(n_nodes: int, a, b, level, n_levels: int) -> np.ndarray:
    """labels[n_levels, n_nodes]: row r = a union-find over the edges with level > r."""
    a, b, level = np.asarray(a), np.asarray(b), np.asarray(level)
    return np.array([union_find(n_nodes, a[level > r], b[level > r]) for r in range(n_levels)], dtype=np.uint32).reshape(n_levels, n_nodes)
