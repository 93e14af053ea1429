"""A plain-Python restatement of the dereplication: the yardstick of tests/test_derep_cpu.py and
tests/test_derep_gpu.py.  The reference has no such tool — its `repr_sketches` stops at the ranking — so nothing
reference-generated can pin the result: this file restates the definition.

    kept      a record whose column passes the text test of `repr_sketches` ('%.6g' text -> strtof -> > threshold) and whose
              ends are nodes; a NaN never passes
    degree    every kept record counts for both of its ends (a repeated pair again, a self pair twice)
    rank      all nodes by (degree descending, node ascending)
    walk      in rank order: a node is a representative unless a kept neighbour of smaller rank is one; otherwise a member
              of the smallest-ranked representative among its kept neighbours, through the lowest-index kept record between
              the two.  Self pairs take no part.

Every value goes through its own text; there is no critical float and there are no rounds here."""
import numpy as np

import repr_restate as rr

NONE = 0xFFFFFFFF


def kept_records(edges, kmer_counts, col, threshold, n_nodes=None):
    """Indices of the kept records, ascending."""
    n = len(kmer_counts) if n_nodes is None else n_nodes
    ok = (edges["source_1"] < n) & (edges["source_2"] < n)
    idx = np.nonzero(ok)[0]
    vals = rr.column_values(edges[idx], kmer_counts, col).tolist()
    return [int(i) for i, v in zip(idx.tolist(), vals) if rr.strtof("%.6g" % v) > threshold]


def select(n_nodes, pairs):
    """pairs: (a, b, index) of the kept records, in index order.  Returns dict(rep, via, rank, degree, n_reps)."""
    degree = [0] * n_nodes
    nbrs = [[] for _ in range(n_nodes)]
    for a, b, i in pairs:
        degree[a] += 1
        degree[b] += 1
        if a != b:
            nbrs[a].append((b, i))
            nbrs[b].append((a, i))
    order = sorted(range(n_nodes), key=lambda v: (-degree[v], v))
    rank = [0] * n_nodes
    for pos, v in enumerate(order):
        rank[v] = pos
    is_rep = [False] * n_nodes
    rep, via = list(range(n_nodes)), [NONE] * n_nodes
    for v in order:
        covering = [(rank[u], i, u) for u, i in nbrs[v] if rank[u] < rank[v] and is_rep[u]]
        if covering:
            _, via[v], rep[v] = min(covering)
        else:
            is_rep[v] = True
    u32 = lambda x: np.array(x, dtype=np.uint32)
    return dict(rep=u32(rep), via=u32(via), rank=u32(rank), degree=u32(degree), n_reps=sum(is_rep))


def dereplicate(edges, kmer_counts, col=4, threshold=0.20, n_nodes=None):
    n = len(kmer_counts) if n_nodes is None else n_nodes
    s1, s2 = edges["source_1"].tolist(), edges["source_2"].tolist()
    return select(n, [(s1[i], s2[i], i) for i in kept_records(edges, kmer_counts, col, threshold, n)])


def render(dist, names, res, texts):
    """The file: names[v] per node, texts[i] the value text of record i."""
    out = [f"source\trepresentative\t{dist}\tneighbours\trank\n"]
    for v, name in enumerate(names):
        r = int(res["rep"][v])
        out.append(f"{name}\t{names[r]}\t{'-' if r == v else texts[int(res['via'][v])]}\t{int(res['degree'][v])}\t{int(res['rank'][v])}\n")
    return "".join(out).encode()


def dereplicated_tsv(tsv_text, names, col=4, threshold=0.20, dist="avg_cont"):
    """What kspider_dereplicate writes for this pairwise TSV: ids are 1-based rows of `names`; `via` counts the kept rows.  A
    field is read without the blanks around it, as the loader of `kSpider cluster` reads it (strip), and printed so."""
    rows = [[x.strip() for x in l.split("\t")] for l in tsv_text.split("\n")[1:] if l]
    kept = [r for r in rows if rr.text_passes(r[col], threshold)]
    res = select(len(names), [(int(r[0]) - 1, int(r[1]) - 1, i) for i, r in enumerate(kept)])
    return render(dist, names, res, [r[col] for r in kept])
