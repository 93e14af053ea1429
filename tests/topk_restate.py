"""The top-k neighbours restated in numpy: the yardstick of tests/test_topk_cpu.py and tests/test_topk_gpu.py.
The reference has no such tool, so nothing reference-generated can pin the result: this file restates the definition.

    entries   an entry of node v is a record that names v and is no self pair; every such record is an entry of both of its
              ends, whatever its `shared`; a repeated pair is listed again; a record naming a node >= n_nodes is ignored
    order     value descending, a NaN below every number, ties by record index, lower first
    value     the float of column 3 / 4 / 5 in single precision (repr_restate.column_values); +inf sorts first
    result    count[v] = min(k, entries of v); index[v, i], i < count[v], the record of the i-th entry; 0xFFFFFFFF behind

One lexsort over all entries by (node, is NaN, -value, index); there is no key, no class and no kernel here.  Nothing in this
file calls the code under test."""
import numpy as np

from repr_restate import column_values

NONE = 0xFFFFFFFF


def select(n_nodes: int, a, b, value, k: int):
    """(index [n_nodes, k] uint32, count [n_nodes] uint32, entries [n_nodes] int64) for records (a[i], b[i]) of value[i]."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    value = np.asarray(value).astype(np.float64)            # (a float32, or an integer below 2^53, is exact in a double)
    rec = np.nonzero((a < n_nodes) & (b < n_nodes) & (a != b))[0]
    node = np.concatenate([a[rec], b[rec]])
    idx = np.concatenate([rec, rec])
    v = np.concatenate([value[rec], value[rec]])
    nan = np.isnan(v)
    order = np.lexsort((idx, np.where(nan, 0.0, -v), nan, node))
    node, idx = node[order], idx[order]
    entries = np.bincount(node, minlength=n_nodes).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(entries)[:-1]]) if n_nodes else np.zeros(0, dtype=np.int64)
    pos = np.arange(len(node)) - start[node]
    keep = pos < k
    index = np.full((n_nodes, k), NONE, dtype=np.uint32)
    index[node[keep], pos[keep]] = idx[keep]
    return index, np.minimum(entries, k).astype(np.uint32), entries


def topk(edges: np.ndarray, kmer_counts: np.ndarray, col: int, k: int, n_nodes: int | None = None):
    """ksp_edges_topk restated: (index, count)."""
    n = len(kmer_counts) if n_nodes is None else n_nodes
    inside = (edges["source_1"] < n) & (edges["source_2"] < n)
    value = np.full(len(edges), np.nan, dtype=np.float32)   # (a record with an end outside is ignored: its value is never used)
    value[inside] = column_values(edges[inside], np.asarray(kmer_counts), col)
    index, count, _ = select(n, edges["source_1"], edges["source_2"], value, k)
    return index, count


def entries(edges: np.ndarray, n_nodes: int) -> np.ndarray:
    """Entries per node."""
    return select(n_nodes, edges["source_1"], edges["source_2"], np.zeros(len(edges)), 1)[2]


def ranked(n_nodes: int, a, b, rank, k: int):
    """ksp_topk_ranked restated: a higher rank is better."""
    index, count, _ = select(n_nodes, a, b, np.asarray(rank).astype(np.float64), k)
    return index, count


def render(dist: str, names: list, a, b, texts: list, index: np.ndarray, count: np.ndarray) -> bytes:
    """The file: rows (a[i], b[i]) are node indices, texts[i] the value text of row i."""
    out = [f"source\thit\tneighbour\t{dist}\n"]
    for v, name in enumerate(names):
        for i in range(int(count[v])):
            e = int(index[v, i])
            other = int(b[e]) if int(a[e]) == v else int(a[e])
            out.append(f"{name}\t{i + 1}\t{names[other]}\t{texts[e]}\n")
    return "".join(out).encode()


def tsv_rows(tsv_text: str) -> list:
    """The data rows of a pairwise TSV, every field without the blanks around it (as the loader of `kSpider cluster` reads them)."""
    return [[x.strip() for x in l.split("\t")] for l in tsv_text.split("\n")[1:] if l.strip()]


def topk_tsv(tsv_text: str, names: list, col: int, k: int, dist: str, texts: list | None = None) -> bytes:
    """What kspider_topk writes for this pairwise TSV: the weight of a row is its text read as a double.  texts: the value texts
    when they are not column col of the TSV (the lines of the ANI column file)."""
    rows = tsv_rows(tsv_text)
    texts = [r[col] for r in rows] if texts is None else [t.strip() for t in texts]
    assert len(texts) == len(rows)
    a, b = [int(r[0]) - 1 for r in rows], [int(r[1]) - 1 for r in rows]
    index, count, _ = select(len(names), a, b, [float(t) for t in texts], k)
    return render(dist, names, a, b, texts, index, count)


def topk_tsv_floats(tsv_text: str, names: list, kmer_counts, col: int, k: int, dist: str) -> bytes:
    """What kspider_pairwise_and_topk writes beside this pairwise TSV: the rows ordered by the FLOAT of their column, computed from
    `shared_kmers` and the k-mer counts of the two sources (kmer_counts[id - 1]), the index of a row its place in the TSV.  The
    text of a row is the TSV's own, which prints that float with 6 digits (checked here for every number)."""
    rows = tsv_rows(tsv_text)
    e = np.zeros(len(rows), dtype=[("source_1", "<u4"), ("source_2", "<u4"), ("shared", "<u8")])
    e["source_1"], e["source_2"], e["shared"] = [int(r[0]) - 1 for r in rows], [int(r[1]) - 1 for r in rows], [int(r[2]) for r in rows]
    value = column_values(e, np.asarray(kmer_counts), col)
    for r, v in zip(rows, value.tolist()):
        assert v != v or "%g" % v == r[col], (r, v)
    index, count, _ = select(len(names), e["source_1"], e["source_2"], value, k)
    return render(dist, names, e["source_1"], e["source_2"], [r[col] for r in rows], index, count)


def per_source(topk_file: bytes) -> dict:
    """{source name: [(neighbour name, value text), ...] in hit order} of a top-k file; the hit numbers are checked to count 1, 2, ..."""
    out = {}
    lines = topk_file.decode().split("\n")
    assert lines[0].startswith("source\thit\tneighbour\t") and lines[-1] == ""
    for line in lines[1:-1]:
        s, hit, nb, text = line.split("\t")
        out.setdefault(s, []).append((nb, text))
        assert int(hit) == len(out[s])
    return out
