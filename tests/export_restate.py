"""Python/numpy restatement of `kSpider export` (pykSpider/kSpider2/ks_export.py) for the tests.

Every step is restated from the behaviour DESIGN.md §7b records: pandas' DataFrame fill and `to_csv`, pandas'
`read_csv` float parser (`precise_xstrtod`), scipy's `linkage(M, 'single')` on a 2-D array (Euclidean `pdist`
between the ROWS, a plain sequential sum, then `mst_single_linkage`: Prim from node 0, a stable sort by height, a
union-find relabel) and the reference's `get_newick`, written without recursion.  Neither pandas nor scipy is used."""
import math
import os

import numpy as np

DIST_COL = {"min_cont": 3, "avg_cont": 4, "max_cont": 5, "ani": None}
E = [float(f"1e{i}") for i in range(309)]


def xstrtod(s):
    """pandas' default float parser (precise_xstrtod) on the text of one cell; not correctly rounded."""
    if s in ("inf", "+inf"):
        return math.inf
    if s == "-inf":
        return -math.inf
    if s == "nan":
        return math.nan
    p, neg = 0, False
    if s[p] in "+-":
        neg = s[p] == "-"
        p += 1
    num, nd, ex, ndec = 0.0, 0, 0, 0
    while p < len(s) and s[p].isdigit():
        if nd < 17:
            num = num * 10.0 + int(s[p])
            nd += 1
        else:
            ex += 1
        p += 1
    if p < len(s) and s[p] == ".":
        p += 1
        while nd < 17 and p < len(s) and s[p].isdigit():
            num = num * 10.0 + int(s[p])
            p += 1
            nd += 1
            ndec += 1
        while p < len(s) and s[p].isdigit():
            p += 1
        ex -= ndec
    if p < len(s) and s[p] in "eE":
        p += 1
        en = s[p] == "-"
        if s[p] in "+-":
            p += 1
        ex += -int(s[p:]) if en else int(s[p:])
    if ex > 308:
        num = math.inf
    elif ex > 0:
        num *= E[ex]
    elif ex < -308:
        num = 0.0 if ex < -616 else num / E[-308 - ex] / E[308]
    else:
        num /= E[-ex]
    return -num if neg else num


def csv_field(name):
    """A field as csv's QUOTE_MINIMAL writes it with sep '\\t' (names hold no blanks: .namesMap is split on them)."""
    return '"' + name.replace('"', '""') + '"' if '"' in name else name


def read_inputs(prefix, dist_type="max_cont"):
    """-> (rows, header): rows = [(name1, name2, value)] in TSV order, as ks_export.main reads them."""
    if dist_type not in DIST_COL:
        raise ValueError("unknown distance")
    with open(f"{prefix}_kSpider_seqToKmersNo.tsv") as f:
        next(f)
        for line in f:
            _, n = tuple(line.strip().split("\t")[1:])
            int(n)
    names = {}
    with open(f"{prefix}.namesMap") as f:
        next(f)
        for line in f:
            p = line.strip().split()
            names[p[0]] = p[1]
    rows = []
    ani = open(f"{prefix}_kSpider_pairwise.ani_col.tsv") if dist_type == "ani" else None
    try:
        if ani:
            next(ani)
        with open(f"{prefix}_kSpider_pairwise.tsv") as f:
            next(f)
            for line in f:
                p = line.strip().split("\t")
                v = float(next(ani).strip()) if ani else float(p[DIST_COL[dist_type]])
                rows.append((names[p[0]], names[p[1]], v))
    finally:
        if ani:
            ani.close()
    header = "source1\tsource2\tani\n" if dist_type == "ani" else f"grp1\tgrp2\t{dist_type}\n"
    return rows, header


def export_texts(rows, header):
    """-> (pairwise text, distmat text, node names, dense matrix M as read back by pandas)."""
    pw = [header] + [f"{a}\t{b}\t{v!r}\n" for a, b, v in rows]
    nodes = sorted({x for a, b, _ in rows for x in (a, b)})
    pos = {x: i for i, x in enumerate(nodes)}
    n = len(nodes)
    cell = {}
    real = [False] * n            # column has an assigned value that is not NaN: float64, else int64 after fillna(0)
    for a, b, v in rows:
        if a == b or (a, b) in cell or (b, a) in cell:
            raise ValueError("self pair or repeated pair")
        cell[(a, b)] = cell[(b, a)] = 1 - v
        if v == v:
            real[pos[a]] = real[pos[b]] = True
    lines = ["\t" + "\t".join(csv_field(x) for x in nodes) + "\n"]
    M = np.zeros((n, n))
    for i, x in enumerate(nodes):
        out = [csv_field(x)]
        for j, y in enumerate(nodes):
            c = cell.get((x, y))
            if c is None or c != c:
                out.append("0.0" if real[j] else "0")
            else:
                t = repr(c)
                out.append(t)
                M[i, j] = xstrtod(t)
        lines.append("\t".join(out) + "\n")
    return "".join(pw), "".join(lines), nodes, M


def row_pdist(M):
    """The full n x n matrix of scipy's pdist(M, 'euclidean'): per pair a sequential sum over the columns, in order,
    then sqrt.  A column where both rows are 0 adds +0 exactly, so column c only touches the pairs with a nonzero in
    it (rows r): S[r, :] += U, and S[:, r] += U.T for the other rows (adding +0 where a pair was already counted)."""
    n = M.shape[0]
    S = np.zeros((n, n))
    for c in range(M.shape[1]):
        r = np.flatnonzero(M[:, c])
        if not len(r):
            continue
        U = M[r, c][:, None] - M[:, c][None, :]
        U *= U                                # numpy: no fused multiply-add
        S[r, :] += U
        Ut = U.T.copy()
        Ut[r, :] = 0.0
        S[:, r] += Ut
    return np.sqrt(S)


def prim_rows(D, nearest=False):
    """scipy's mst_single_linkage before the sort: (x, y, height) per step, ties to the smallest index; with nearest
    also the merged node whose row last lowered D[y] (`if D[i] > d`), i.e. height = D[m, y]."""
    n = D.shape[0]
    merged = np.zeros(n, dtype=bool)
    Dm = np.full(n, np.inf)
    near = np.zeros(n, dtype=np.int64)
    out = np.empty((n - 1, 4))
    x = 0
    for k in range(n - 1):
        merged[x] = True
        lower = ~merged & (Dm > D[x])
        Dm[lower] = D[x, lower]
        near[lower] = x
        cand = np.where(merged, np.inf, Dm)
        y = int(np.argmin(cand))           # argmin: first index of the minimum
        out[k] = (x, y, cand[y], near[y])
        x = y
    return out if nearest else out[:, :3]


def relabel(rows, n):
    """Stable sort by height and union-find relabel: scipy's linkage matrix Z."""
    order = np.argsort(rows[:, 2], kind="mergesort")
    rows = rows[order]
    parent = list(range(2 * n - 1))
    size = [1] * n + [0] * (n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:          # path compression: a chain of n merges stays O(n), not O(n^2)
            parent[x], x = r, parent[x]
        return r

    Z = np.empty((n - 1, 4))
    for i in range(n - 1):
        a, b = find(int(rows[i, 0])), find(int(rows[i, 1]))
        lo, hi = min(a, b), max(a, b)
        parent[a] = parent[b] = n + i
        size[n + i] = size[a] + size[b]
        Z[i] = (lo, hi, rows[i, 2], size[n + i])
    return Z


def linkage_rows(M):
    """== scipy.cluster.hierarchy.linkage(M, 'single') for a finite 2-D M, bit for bit."""
    M = np.asarray(M, dtype=np.float64)
    return relabel(prim_rows(row_pdist(M)), M.shape[0])


def newick(Z, names):
    """The reference's to_tree + get_newick text, iteratively: a node prints (<right>,<left>):%.2f, the root ends ');'."""
    n = len(names)
    left = {n + i: int(Z[i, 0]) for i in range(n - 1)}
    right = {n + i: int(Z[i, 1]) for i in range(n - 1)}
    height = {n + i: float(Z[i, 2]) for i in range(n - 1)}
    root = 2 * n - 2
    out = []
    stack = [("node", root, height[root])]
    while stack:
        op = stack.pop()
        if op[0] == "text":
            out.append(op[1])
            continue
        _, v, pd = op
        if v < n:
            out.append("%s:%.2f" % (names[v], pd - 0.0))
            continue
        h = height[v]
        tail = ");" if v == root else "):%.2f" % (pd - h)
        stack += [("text", tail), ("node", left[v], h), ("text", ","), ("node", right[v], h), ("text", "(")]
    return "".join(out)


def export(prefix, dist_type="max_cont", newick_too=False):
    """-> {suffix: text}: the files `kSpider export -i PREFIX -d DIST [--newick]` writes ('_pairwise.tsv',
    '_distmat.tsv', '.newick')."""
    rows, header = read_inputs(prefix, dist_type)
    pw, dm, nodes, M = export_texts(rows, header)
    out = {"_pairwise.tsv": pw, "_distmat.tsv": dm}
    if newick_too:
        if len(nodes) < 2 or not np.isfinite(M).all():
            raise ValueError("newick needs 2 nodes and finite values")
        out[".newick"] = newick(linkage_rows(M), nodes)
    return out


def default_names(prefix):
    b = os.path.basename(prefix)
    return {"_pairwise.tsv": f"kSpider_{b}_pairwise.tsv", "_distmat.tsv": f"kSpider_{b}_distmat.tsv",
            ".newick": f"kSpider_{b}.newick"}
