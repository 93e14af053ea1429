"""The average-linkage tree (UPGMA) of include/kspider_amd.h restated for the tests, independent of the product's code.

sequential_small   the definition in Python integers and Fractions over a dict of pairs: O(n * m), small inputs only.
parallel_small     the parallel form of DESIGN.md 7m (every cluster picks its first pair, mutual picks merge at once, the rest is
                   contracted, rows sorted at the end), the same way: the theorem is that both give the same rows.
merges             the same sequential definition — the globally first pair, again and again — with numpy arrays, so that the GPU
                   tests' inputs (thousands of nodes) take seconds: the first pair is found among the pairs whose float64
                   similarity is within 1e-12 of the largest, by exact 128-bit cross products (two 64-bit limbs).  trunc=True keeps
                   only the low 64 bits of every cross product, in the choice of the first pair and when the rows are put in order at
                   the end (the device orders its rows at the end by the same comparison): used only to prove that an input is hostile.
Also the file writers: the merge table, the newick text and the clusters of a cut."""
from fractions import Fraction

import numpy as np

TWO32 = 4294967296
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
ROW_DTYPE = np.dtype([("lo", "<u4"), ("hi", "<u4"), ("sum_q", "<u8"), ("size_lo", "<u4"), ("size_hi", "<u4")])


def q_of(value) -> np.ndarray:
    """q(v) = (uint64_t)((double)v * 2^32) for floats in [0, 1]; 0 for a NaN and anything outside (those take no part / are refused)."""
    v = np.ascontiguousarray(value, dtype=np.float32).astype(np.float64)
    ok = (v >= 0) & (v <= 1)
    return np.where(ok, np.floor(np.where(ok, v, 0.0) * float(TWO32)), 0).astype(np.uint64)


def pairs_of(n_nodes, a, b, q) -> dict:
    """{(lo, hi): S} over the records that take part."""
    S = {}
    for x, y, w in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(q).tolist()):
        if x >= n_nodes or y >= n_nodes or x == y or w == 0:
            continue
        k = (min(x, y), max(x, y))
        S[k] = S.get(k, 0) + w
    return S


def order_key(row):
    """Sort key of a row (lo, hi, S, size_lo, size_hi) in the order of candidate pairs."""
    return (-Fraction(row[2], row[3] * row[4]), row[0], row[1])


def before(p1, p2, bits=None) -> bool:
    """Pair (S, size_lo, size_hi, lo, hi) p1 before p2; bits: keep only that many low bits of each cross product."""
    x, y = p1[0] * p2[1] * p2[2], p2[0] * p1[1] * p1[2]
    if bits:
        x, y = x & ((1 << bits) - 1), y & ((1 << bits) - 1)
    if x != y:
        return x > y
    return (p1[3], p1[4]) < (p2[3], p2[4])


def _relabel(S, lab):
    T = {}
    for (x, y), w in S.items():
        x2, y2 = lab.get(x, x), lab.get(y, y)
        if x2 != y2:
            k = (min(x2, y2), max(x2, y2))
            T[k] = T.get(k, 0) + w
    return T


def sequential_small(n_nodes, a, b, q) -> list:
    S = pairs_of(n_nodes, a, b, q)
    size = [1] * n_nodes
    rows = []
    while S:
        lo, hi = min(S, key=lambda p: (-Fraction(S[p], size[p[0]] * size[p[1]]), p[0], p[1]))
        rows.append((lo, hi, S[lo, hi], size[lo], size[hi]))
        S = _relabel(S, {hi: lo})
        size[lo] += size[hi]
    return rows


def parallel_small(n_nodes, a, b, q):
    """(rows, rounds, the longest run of equal pairs a contraction summed)."""
    S = pairs_of(n_nodes, a, b, q)
    size = [1] * n_nodes
    rows, rounds, longest = [], 0, 0
    while S:
        rounds += 1
        pick = {}
        for p in S:
            k = (-Fraction(S[p], size[p[0]] * size[p[1]]), p[0], p[1])
            for c in p:
                if c not in pick or k < pick[c][0]:
                    pick[c] = (k, p)
        merged = sorted({p for _, p in pick.values() if pick[p[0]][1] == p and pick[p[1]][1] == p})
        assert merged, "a round with a candidate merges at least one pair"
        rows += [(lo, hi, S[lo, hi], size[lo], size[hi]) for lo, hi in merged]
        lab = {hi: lo for lo, hi in merged}
        runs = {}
        for (x, y) in S:
            x2, y2 = lab.get(x, x), lab.get(y, y)
            if x2 != y2:
                k = (min(x2, y2), max(x2, y2))
                runs[k] = runs.get(k, 0) + 1
        longest = max([longest] + list(runs.values()))
        S = _relabel(S, lab)
        for lo, hi in merged:
            size[lo] += size[hi]
    rows.sort(key=order_key)
    return rows, rounds, longest


def _mul128(x, y: int):
    """(high, low) 64-bit limbs of x[i] * y; x a uint64 array, 0 <= y < 2^64."""
    x = x.astype(np.uint64)
    y1, y0 = np.uint64(y >> 32), np.uint64(y & 0xFFFFFFFF)
    x1, x0 = x >> _S32, x & _M32
    ll, m1, m2, hh = x0 * y0, x1 * y0, x0 * y1, x1 * y1
    t = (ll >> _S32) + (m1 & _M32) + (m2 & _M32)
    return hh + (m1 >> _S32) + (m2 >> _S32) + (t >> _S32), (ll & _M32) | ((t & _M32) << _S32)


def _first(S, P, lo, hi, trunc):
    """Index of the first pair in the order."""
    if trunc:
        cand = np.arange(len(S))
    else:
        f = S.astype(np.float64) / P.astype(np.float64)
        cand = np.flatnonzero(f >= f.max() * (1 - 1e-12))
    while True:
        p = cand[0]
        xh, xl = _mul128(S[cand], int(P[p]))
        yh, yl = _mul128(P[cand], int(S[p]))
        if trunc:
            xh = yh = np.zeros(len(cand), dtype=np.uint64)
        better = (xh > yh) | ((xh == yh) & (xl > yl))
        if better.any():
            cand = cand[better]                                          # (the pivot is not among them: the list shrinks)
            continue
        cand = cand[(xh == yh) & (xl == yl)]
        return cand[np.lexsort((hi[cand], lo[cand]))[0]]


def _fold(lo, hi, S):
    key = (lo.astype(np.uint64) << _S32) | hi.astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(u), dtype=np.uint64)
    np.add.at(s, inv, S)
    return (u >> _S32).astype(np.int64), (u & _M32).astype(np.int64), s


def merges(n_nodes, a, b, q, trunc=False) -> np.ndarray:
    """The rows of the sequential definition, as a structured array of ROW_DTYPE."""
    a, b, q = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64), np.asarray(q, dtype=np.uint64)
    part = (a < n_nodes) & (b < n_nodes) & (a != b) & (q > 0)
    lo, hi, S = _fold(np.minimum(a, b)[part], np.maximum(a, b)[part], q[part])
    size = np.ones(max(n_nodes, 1), dtype=np.uint64)
    rows = []
    while len(S):
        i = _first(S, size[lo] * size[hi], lo, hi, trunc)
        l, h = int(lo[i]), int(hi[i])
        rows.append((l, h, int(S[i]), int(size[l]), int(size[h])))
        size[l] += size[h]
        keep = np.ones(len(S), dtype=bool)
        keep[i] = False
        touch = keep & ((lo == h) | (hi == h) | (lo == l) | (hi == l))
        rest = keep & ~touch
        tl, th = np.where(lo[touch] == h, l, lo[touch]), np.where(hi[touch] == h, l, hi[touch])
        fl, fh, fs = _fold(np.minimum(tl, th), np.maximum(tl, th), S[touch])
        lo, hi, S = np.concatenate([lo[rest], fl]), np.concatenate([hi[rest], fh]), np.concatenate([S[rest], fs])
    if trunc and rows:                                                   # the device orders its rows at the end by the same comparison:
        r = np.array(rows, dtype=ROW_DTYPE)                              # here by taking the first of the remaining rows, again and again
        left, out = np.arange(len(r)), []
        while len(left):
            x = r[left]
            i = _first(x["sum_q"], x["size_lo"].astype(np.uint64) * x["size_hi"].astype(np.uint64), x["lo"].astype(np.int64), x["hi"].astype(np.int64), True)
            out.append(left[i])
            left = np.delete(left, i)
        return r[np.array(out)]
    return np.array(rows, dtype=ROW_DTYPE) if rows else np.zeros(0, dtype=ROW_DTYPE)


def rows_of(tuples) -> np.ndarray:
    return np.array([tuple(r) for r in tuples], dtype=ROW_DTYPE) if len(tuples) else np.zeros(0, dtype=ROW_DTYPE)


def same(got, want, what=""):
    assert got.dtype == ROW_DTYPE and len(got) == len(want), (what, len(got), len(want))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, int(bad[0]), got[bad[0]], want[bad[0]])


# ---- the files ---------------------------------------------------------------------------------------------------------------

def average(row) -> float:
    return float(int(row["sum_q"])) / (float(int(row["size_lo"])) * float(int(row["size_hi"]))) / float(TWO32)


def table_text(dist, rows) -> str:
    out = [f"source_1\tsource_2\t{dist}_average\tsum_q\tsize_1\tsize_2\tmerged_size\n"]
    for r in rows:
        out.append("%d\t%d\t%.9g\t%d\t%d\t%d\t%d\n" % (int(r["lo"]) + 1, int(r["hi"]) + 1, average(r), int(r["sum_q"]), int(r["size_lo"]), int(r["size_hi"]),
                                                     int(r["size_lo"]) + int(r["size_hi"])))
    return "".join(out)


def newick_text(names, rows) -> str:
    """kspider_tree's conventions: height of a merge 1 - average clamped to [0, 1], branch lengths '%.6g', the child holding lo first,
    clusters that never join under one root at height 1 in order of their smallest node."""
    body = {v: (names[v], 0.0) for v in range(len(names))}                  # root -> (text without a branch length, height)
    for r in rows:
        lo, hi = int(r["lo"]), int(r["hi"])
        h = min(1.0, max(0.0, 1.0 - average(r)))
        (tl, hl), (th, hh) = body[lo], body.pop(hi)
        body[lo] = ("(%s:%s,%s:%s)" % (tl, "%.6g" % (h - hl), th, "%.6g" % (h - hh)), h)
    roots = [body[v] for v in sorted(body)]
    if not roots:
        return ";\n"
    if len(roots) == 1:
        return roots[0][0] + ";\n"
    return "(" + ",".join("%s:%s" % (t, "%.6g" % (1.0 - h)) for t, h in roots) + ");\n"


def cut_labels(n_nodes, rows, cutoff) -> list:
    """label[v] = the smallest member of v's cluster when the rows whose average is at least the cut-off are kept (exactly:
    sum_q >= floor(cutoff * 2^32) * size_lo * size_hi)."""
    q_cut = int(cutoff * float(TWO32))
    parent = list(range(n_nodes))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for r in rows:
        if int(r["sum_q"]) >= q_cut * int(r["size_lo"]) * int(r["size_hi"]):
            x, y = find(int(r["lo"])), find(int(r["hi"]))
            if x != y:
                parent[max(x, y)] = min(x, y)
    return [find(v) for v in range(n_nodes)]


def cluster_text(names, label) -> str:
    members = {}
    for v, r in enumerate(label):
        members.setdefault(r, []).append(names[v])
    return "".join(",".join(members[r]) + "\n" for r in sorted(members))


def read_table(text, dist) -> np.ndarray:
    lines = text.split("\n")
    assert lines[0] == f"source_1\tsource_2\t{dist}_average\tsum_q\tsize_1\tsize_2\tmerged_size" and lines[-1] == ""
    rows = []
    for l in lines[1:-1]:
        p = l.split("\t")
        assert len(p) == 7 and int(p[4]) + int(p[5]) == int(p[6])
        rows.append((int(p[0]) - 1, int(p[1]) - 1, int(p[3]), int(p[4]), int(p[5])))
    return rows_of(rows)
