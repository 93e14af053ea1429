"""The single-linkage tree restated (tests only): Kruskal over the SAME strict total order the device uses — the column value
as a float, larger first, a NaN above every number, ties by record index, lower first.  The order is strict, so the maximum
spanning forest is unique: what comes back here is the one and only forest, in merge order, and the device's indices are
compared with it element for element.  Values come from repr_restate.column_values, cuts from sweep_restate / cut_restate.
Nothing here calls the code under test."""
import numpy as np

from repr_restate import column_values

NAN_KEY = 0xFFFFFFFF


def keys(edges: np.ndarray, kmer_counts: np.ndarray, col: int) -> np.ndarray:
    """Per record the 32-bit key of its column value: the float's bit pattern (no value is negative, so it is monotone), a NaN the top."""
    v = column_values(edges, np.asarray(kmer_counts), col).astype(np.float32)
    k = v.view(np.uint32).astype(np.int64)
    assert (k[~np.isnan(v)] <= 0x7F800000).all(), "a negative value"
    k[np.isnan(v)] = NAN_KEY
    return k


def kruskal(n_nodes: int, a, b, key) -> np.ndarray:
    """Indices of the forest's edges in merge order: key descending, then index ascending; an edge with a == b never merges."""
    a, b, key = np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(key, dtype=np.int64)
    order = np.lexsort((np.arange(len(key)), -key)).tolist()
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    for e in order:
        ra, rb = find(a[e]), find(b[e])
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append(e)
    return np.array(out, dtype=np.uint32)


def forest(n_nodes: int, edges: np.ndarray, kmer_counts: np.ndarray, col: int) -> np.ndarray:
    return kruskal(n_nodes, edges["source_1"], edges["source_2"], keys(edges, kmer_counts, col))


def weight_key(text: str):
    """Sort key of a row's text on the file path: the value kspider_cluster tests, float(text) * 100, larger first, a NaN on top."""
    w = float(text) * 100
    return (0, 0.0) if w != w else (1, -w)


def tree_rows(n_nodes: int, rows: list) -> list:
    """rows: (id_1, id_2, text) of a pairwise TSV.  -> the rows of the tree file: Kruskal by (weight_key, row index), then the chosen
    rows in the file's order — weight descending (NaN first), then (id_1, id_2) — each with the size of the cluster its merge makes."""
    order = sorted(range(len(rows)), key=lambda i: (weight_key(rows[i][2]), i))
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    chosen = []
    for i in order:
        ra, rb = find(rows[i][0] - 1), find(rows[i][1] - 1)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            chosen.append(rows[i])
    chosen.sort(key=lambda r: (weight_key(r[2]), r[0], r[1]))
    parent, size, out = list(range(n_nodes)), [1] * n_nodes, []
    for a, b, text in chosen:
        ra, rb = find(a - 1), find(b - 1)
        assert ra != rb
        lo, hi = min(ra, rb), max(ra, rb)
        parent[hi] = lo
        size[lo] += size[hi]
        out.append((a, b, text, size[lo]))
    return out


def tree_tsv(dist: str, n_nodes: int, rows: list) -> str:
    return f"source_1\tsource_2\t{dist}\tmerged_size\n" + "".join(f"{a}\t{b}\t{t}\t{s}\n" for a, b, t, s in tree_rows(n_nodes, rows))


def parse_newick(text: str):
    """-> (leaves: {name: root-to-leaf sum of branch lengths}, lengths: every branch length).  The root carries no length."""
    assert text.endswith(";\n")
    s, pos, leaves, lengths = text[:-2], 0, {}, []
    stack = [[]]                       # per open bracket: the subtrees read so far, each a list of [name, depth below this bracket]
    while pos < len(s):
        ch = s[pos]
        if ch == "(":
            stack.append([])
            pos += 1
        elif ch == ",":
            pos += 1
        else:
            if ch == ")":
                sub = [leaf for child in stack.pop() for leaf in child]
                pos += 1
            else:
                end = pos
                while end < len(s) and s[end] not in ",():":
                    end += 1
                sub, pos = [[s[pos:end], 0.0]], end
            if pos < len(s) and s[pos] == ":":
                end = pos + 1
                while end < len(s) and s[end] not in ",()":
                    end += 1
                length, pos = float(s[pos + 1:end]), end
                lengths.append(length)
                for leaf in sub:
                    leaf[1] += length
            stack[-1].append(sub)
    assert len(stack) == 1 and len(stack[0]) == 1
    for name, depth in stack[0][0]:
        assert name not in leaves
        leaves[name] = depth
    return leaves, lengths
