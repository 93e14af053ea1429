"""The cluster report restated (tests only; the definitions of include/kspider_amd.h, "the cluster report"): a union-find for the
labels, q = floor(v * 2^32) by integer arithmetic on the float's exact value, sums in unsigned 64-bit integers, the medoid by
(strength descending, node ascending), via as the lowest kept index between a member and its medoid, and the two files.  Nothing
here calls the code under test; which records `kSpider cluster` keeps comes from tests/cut_restate.py, through the text."""
from fractions import Fraction

import numpy as np

import cut_restate as cr
import repr_restate as rr
from kspider_amd import engine

NONE = 0xFFFFFFFF
CLUSTER = engine.CLUSTER_ROW_DTYPE
MEMBER = engine.MEMBER_ROW_DTYPE
REPORT_HEADER = "cluster\tsize\tedges\tdensity\tmin\tmean\tmax\tmedoid\tmedoid_strength\tcovered\n"


def q_exact(v) -> int:
    """floor(v * 2^32) of a float32 in [0, 1], through the exact fraction the float is."""
    f = Fraction(float(np.float32(v)))
    assert 0 <= f <= 1
    return (f.numerator << 32) // f.denominator


def q_of(values: np.ndarray) -> np.ndarray:
    """q_exact of every value (none is a NaN), asked once per distinct value."""
    distinct, place = np.unique(values, return_inverse=True)
    table = np.array([q_exact(v) for v in distinct.tolist()], dtype=np.uint64)
    return table[place] if len(values) else np.zeros(0, dtype=np.uint64)


def labels_of(n_nodes: int, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """label[v] = smallest node of v's component: a union-find over the distinct pairs."""
    lo, hi = np.minimum(a, b).astype(np.uint64), np.maximum(a, b).astype(np.uint64)
    pairs = np.unique((lo << np.uint64(32)) | hi)
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p in pairs.tolist():
        ru, rv = find(p >> 32), find(p & 0xFFFFFFFF)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(v) for v in range(n_nodes)], dtype=np.uint32)


def report(n_nodes: int, a, b, values, index=None):
    """(cluster rows, member rows) of the records (a[i], b[i], values[i]), ALL of which passed the cut; index[i]: the record's index
    in the caller's list (default: i).  A record naming a node >= n_nodes and a self pair take no part."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    values = np.asarray(values, dtype=np.float32)
    index = np.arange(len(a), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    part = (a < n_nodes) & (b < n_nodes) & (a != b)
    a, b, values, index = a[part], b[part], values[part], index[part]
    nan = np.isnan(values)
    assert ((values[~nan] >= 0) & (values[~nan] <= 1)).all(), "outside the domain: the call is refused"
    q = np.zeros(len(a), dtype=np.uint64)
    q[~nan] = q_of(values[~nan])
    label = labels_of(n_nodes, a, b)
    member = np.zeros(n_nodes, dtype=MEMBER)
    member["label"] = label
    member["degree"] = np.bincount(a, minlength=n_nodes) + np.bincount(b, minlength=n_nodes)
    strength = np.zeros(n_nodes, dtype=np.uint64)
    np.add.at(strength, a, q)
    np.add.at(strength, b, q)
    member["strength"] = strength
    of = label[a]                                                      # the cluster of every record
    edges, nans, sum_q = (np.zeros(n_nodes, dtype=np.uint64) for _ in range(3))
    np.add.at(edges, of, np.uint64(1))
    np.add.at(nans, of[nan], np.uint64(1))
    np.add.at(sum_q, of, q)
    mn, mx = np.full(n_nodes, np.inf, dtype=np.float32), np.full(n_nodes, -np.inf, dtype=np.float32)
    np.minimum.at(mn, of[~nan], values[~nan])
    np.maximum.at(mx, of[~nan], values[~nan])
    valued = edges > nans
    mn[~valued] = mx[~valued] = np.nan
    # the medoid: the first member of every cluster by (strength descending, node ascending)
    order = np.lexsort((np.arange(n_nodes), ~strength, label))
    first = np.ones(n_nodes, dtype=bool)
    first[1:] = label[order][1:] != label[order][:-1]
    medoid = np.zeros(n_nodes, dtype=np.int64)
    medoid[label[order][first]] = order[first]
    # via: the lowest index of a record between a member and its medoid
    m = medoid[of]
    via = np.full(n_nodes, NONE, dtype=np.int64)
    np.minimum.at(via, b[a == m], index[a == m])
    np.minimum.at(via, a[b == m], index[b == m])
    member["via"] = via
    roots = np.nonzero(label == np.arange(n_nodes))[0]
    cluster = np.zeros(len(roots), dtype=CLUSTER)
    cluster["root"] = roots
    cluster["size"] = np.bincount(label, minlength=n_nodes)[roots]
    cluster["edges"], cluster["nan_edges"], cluster["sum_q"] = edges[roots], nans[roots], sum_q[roots]
    cluster["min"], cluster["max"] = mn[roots], mx[roots]
    cluster["medoid"] = medoid[roots]
    cluster["covered"] = np.bincount(label[via != NONE], minlength=n_nodes)[roots]
    return cluster, member


def kept_mask(e: np.ndarray, cnt: np.ndarray, col: int, cutoff: float, n_nodes: int) -> np.ndarray:
    """The records `kSpider cluster` keeps at this cut-off, through the text of their own value (cut_restate.keep); a record naming a
    node >= n_nodes has no value and is not kept."""
    inside = (e["source_1"] < n_nodes) & (e["source_2"] < n_nodes)
    mask = np.zeros(len(e), dtype=bool)
    v = rr.column_values(e[inside], np.asarray(cnt), col)
    distinct, place = np.unique(v.view(np.uint32), return_inverse=True)
    table = np.array([cr.keep("%.6g" % float(x), cutoff) for x in distinct.view(np.float32).tolist()], dtype=bool).reshape(len(distinct))
    mask[inside] = table[place]
    return mask


def report_edges(e: np.ndarray, cnt: np.ndarray, col: int, cutoff: float, n_nodes: int):
    """What ksp_edges_cluster_report returns for these records, or None when it refuses them (a kept value above 1)."""
    mask = kept_mask(e, cnt, col, cutoff, n_nodes) & (e["source_1"] != e["source_2"])
    k = np.nonzero(mask)[0]
    v = rr.column_values(e[k], np.asarray(cnt), col)
    if (v[~np.isnan(v)] > 1).any():
        return None
    return report(n_nodes, e["source_1"][k], e["source_2"][k], v, k)


def same(got, want, what, via=True):
    """Exact equality of both tables (a NaN equals a NaN)."""
    for name, g, w in (("cluster", got[0], want[0]), ("member", got[1], want[1])):
        assert len(g) == len(w), (what, name, len(g), len(w))
        for field in g.dtype.names:
            if field == "via" and not via:
                continue
            eq = np.array_equal(g[field], w[field], equal_nan=True) if g[field].dtype.kind == "f" else np.array_equal(g[field], w[field])
            assert eq, (what, name, field, np.nonzero(g[field] != w[field])[0][:5].tolist())


# ---- the files -----------------------------------------------------------------------------------------------------------------

def g6(x: float) -> str:
    return "%.6g" % x


def file_tail(dist: str, cutoff: float) -> str:
    return f"_{dist}_{cutoff * 100.0!r}%.tsv"


def files(cluster, member, names, via_text, dist: str):
    """(the cluster report, the members' table) as bytes."""
    number = {int(c["root"]): i + 1 for i, c in enumerate(cluster)}
    out = [REPORT_HEADER]
    for i, c in enumerate(cluster):
        size, edges, valued = int(c["size"]), int(c["edges"]), int(c["edges"]) - int(c["nan_edges"])
        density = g6(edges / (size * (size - 1) / 2)) if size > 1 else "-"
        mean = g6(int(c["sum_q"]) / valued / 2.0**32) if valued else "-"
        lo, hi = ("-" if np.isnan(c[k]) else g6(float(c[k])) for k in ("min", "max"))
        out.append(f"{i + 1}\t{size}\t{edges}\t{density}\t{lo}\t{mean}\t{hi}\t{names[int(c['medoid'])]}\t"
                   f"{g6(int(member['strength'][int(c['medoid'])]) / 2.0**32)}\t{int(c['covered'])}\n")
    rows = [f"source\tcluster\tmedoid\t{dist}\tneighbours\tstrength\n"]
    for v, m in enumerate(member):
        k = number[int(m["label"])]
        rows.append(f"{names[v]}\t{k}\t{names[int(cluster[k - 1]['medoid'])]}\t{via_text[v] if int(m['via']) != NONE else '-'}\t{int(m['degree'])}\t"
                    f"{g6(int(m['strength']) / 2.0**32)}\n")
    return "".join(out).encode(), "".join(rows).encode()


def tsv_rows(tsv_text: str) -> list:
    return [line.split("\t") for line in tsv_text.split("\n")[1:] if line]


def report_tsv(tsv_text: str, names: list, col: int, cutoff: float, dist: str, counts=None):
    """What kspider_cluster_report writes for this TSV: the rows kept by the text, their value the text read with strtof.  counts
    (k-mer counts per id - 1): the value is the writer's float of the row instead, as kspider_pairwise_and_cluster_report sums it.
    Returns (report bytes, members bytes, cluster rows, member rows)."""
    rows = [r for r in tsv_rows(tsv_text) if cr.keep(r[col], cutoff)]
    a = np.array([int(r[0]) - 1 for r in rows], dtype=np.int64)
    b = np.array([int(r[1]) - 1 for r in rows], dtype=np.int64)
    text = [r[col] for r in rows]
    if counts is None:
        v = np.array([rr.strtof(t) for t in text], dtype=np.float32)
    else:
        e = np.zeros(len(rows), dtype=engine.EDGE_DTYPE)
        e["source_1"], e["source_2"], e["shared"] = a, b, [int(r[2]) for r in rows]
        v = rr.column_values(e, np.asarray(counts, dtype=np.uint32), col)
        assert all(g6(float(x)) == t for x, t in zip(v.tolist(), text) if x == x)
    cluster, member = report(len(names), a, b, v)
    via_text = [text[int(m["via"])] if int(m["via"]) != NONE else "" for m in member]
    return files(cluster, member, names, via_text, dist) + (cluster, member)


def cluster_file_lines(cluster, member, names) -> list:
    """The lines of kspider_cluster's file: one per cluster in root order, the members' names in node order."""
    lines = {int(c["root"]): [] for c in cluster}
    for v, m in enumerate(member):
        lines[int(m["label"])].append(names[v])
    return [",".join(lines[int(c["root"])]) for c in cluster]
