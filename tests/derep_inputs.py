"""Inputs of the dereplication tests, built once for tests/test_derep_cpu.py (which checks their shapes without a GPU) and
tests/test_derep_gpu.py: graphs as ksp_edge records over sources of COUNT k-mers each, so that shared / COUNT is exact and is
the value of all three columns; the four consequences of the definition as predicates; and a simulation of the rounds of
DESIGN.md §7h (every read sees the latest write), which gives the live pairs after every round."""
import numpy as np

EDGE_DTYPE = np.dtype([("source_1", "<u4"), ("source_2", "<u4"), ("shared", "<u8")])
COUNT = 1 << 20
KEEP, DROP = COUNT // 2, COUNT // 10          # 0.5 passes the text test at 0.20, 0.1 does not
NONE = 0xFFFFFFFF


def edges(s1, s2, shared=None):
    e = np.zeros(len(s1), dtype=EDGE_DTYPE)
    e["source_1"], e["source_2"] = s1, s2
    e["shared"] = KEEP if shared is None else shared
    return e


def same(n):
    return np.full(n, COUNT, dtype=np.uint32)


def path(n, order="ascending", seed=0):
    """A path 0 - 1 - ... - n-1: ids ascending, reversed (every record names the larger id first, last record first), or the
    records in a random permutation."""
    i = np.arange(n - 1)
    if order == "ascending":
        return edges(i, i + 1)
    if order == "reversed":
        return edges((i + 1)[::-1], i[::-1])
    p = np.random.default_rng(seed).permutation(n - 1)
    return edges(i[p], i[p] + 1)


def disjoint_paths(total_pairs, path_pairs=8):
    """(n_nodes, edges): paths of path_pairs records each, and one shorter path for the rest: total_pairs records, all kept, no
    self pair — so the live pairs after the first round are exactly total_pairs (every pair stamps its hi in round 1)."""
    s1, node = [], 0
    left = total_pairs
    while left:
        k = min(path_pairs, left)
        s1.extend(range(node, node + k))
        node += k + 1
        left -= k
    s1 = np.array(s1, dtype=np.int64)
    return node, edges(s1, s1 + 1)


def star(leaves, centre_first=True):
    c = np.zeros(leaves, dtype=np.int64)
    l = 1 + np.arange(leaves)
    return edges(c, l) if centre_first else edges(l, c)


def clique(n):
    a, b = np.triu_indices(n, 1)
    return edges(a, b)


# the "later, smaller-ranked representative" case: h = 0, u1 = 1, u2 = 2, c2 = 3, c1 = 4, then leaves that set the degrees
LATER = dict(h=0, u1=1, u2=2, c2=3, c1=4)


def later_smaller_rep():
    """(n_nodes, edges).  Degrees c1 10 > c2 9 > u2 8 > u1 7 > h 2 > leaves 1, so the ranks are c1, c2, u2, u1, h.  Round 1: c1 and
    u1 are IN (no neighbour of smaller rank).  u1 knocks h OUT in round 2; c1 knocks c2 OUT, and only then is u2 — of smaller
    rank than u1 — free to become IN.  h belongs to u2."""
    h, u1, u2, c2, c1 = 0, 1, 2, 3, 4
    s1, s2 = [u1, u2, c2, c1], [h, h, u2, c2]
    node = 5
    for centre, leaves in ((c1, 9), (c2, 7), (u2, 6), (u1, 6)):
        for _ in range(leaves):
            s1.append(centre)
            s2.append(node)
            node += 1
    return node, edges(s1, s2)


def simulate_rounds(n_nodes, pairs_ab):
    """The rounds over the kept non-self pairs (a, b), every read seeing the latest write.  Returns (is_rep list, live pairs after
    every round): a pair is live after a round when both of its ends were UNDECIDED in that round's pair pass."""
    degree = [0] * n_nodes
    for a, b in pairs_ab:
        degree[a] += 1
        degree[b] += 1
    order = sorted(range(n_nodes), key=lambda v: (-degree[v], v))
    rank = {v: i for i, v in enumerate(order)}
    live = [(a, b) if rank[a] < rank[b] else (b, a) for a, b in pairs_ab if a != b]
    U, IN, OUT = 0, 1, 2
    state, blocked, lives = [U] * n_nodes, [0] * n_nodes, []
    rnd = 0
    while any(s == U for s in state):
        rnd += 1
        assert rnd <= n_nodes + 1
        nxt = []
        for lo, hi in live:
            if state[hi] != U:
                continue
            if state[lo] == IN:
                state[hi] = OUT
            elif state[lo] == U:
                blocked[hi] = rnd
                nxt.append((lo, hi))
        for v in range(n_nodes):
            if state[v] == U and blocked[v] != rnd:
                state[v] = IN
        live = nxt
        lives.append(len(live))
    return [s == IN for s in state], lives


def consequences(n_nodes, e, kept, res):
    """The four consequences of the definition that do not need the restatement (the fourth, order independence, needs two
    runs: see permuted()).  kept: indices of the kept records."""
    rep, via, degree = res["rep"], res["via"], res["degree"]
    is_rep = rep == np.arange(n_nodes)
    s1, s2 = e["source_1"][kept], e["source_2"][kept]
    real = s1 != s2
    assert not (is_rep[s1[real]] & is_rep[s2[real]]).any(), "two representatives share a kept record"
    members = np.nonzero(~is_rep)[0]
    kept_set = set(int(i) for i in kept)
    for v in members.tolist():
        i = int(via[v])
        assert i in kept_set and {int(e["source_1"][i]), int(e["source_2"][i])} == {v, int(rep[v])}, ("a member without a kept record to its representative", v)
        assert is_rep[rep[v]]
    assert is_rep[degree == 0].all(), "a node of degree 0 is no representative"
    assert (via[is_rep] == NONE).all() and int(is_rep.sum()) == res["n_reps"]


def boundary_case(col):
    """(k-mer counts, 4 records) for column col (3 min, 4 avg, 5 max) at threshold 0.20, the two ends of every record counting
    different numbers of k-mers: a value below 0.2f that prints "0.2" (passes), one that prints "0.199999" (fails), a NaN (two
    sources of 0 k-mers: fails) and a plain pass.  `shared` of the first two is searched for, downwards from the value 0.2."""
    import repr_restate as rr
    cnt = np.array([10**7, 6 * 10**6, 10**7, 6 * 10**6, 0, 0, 8, 5], dtype=np.uint32)
    n1, n2 = 10.0**7, 6.0 * 10**6
    top = int(0.2 * {3: max(n1, n2), 5: min(n1, n2), 4: 2.0 / (1.0 / n1 + 1.0 / n2)}[col]) + 2
    found = {}
    for sh in range(top, top - 60, -1):
        v = rr.column_values(edges([0], [1], [sh]), cnt, col)[0]
        text = "%.6g" % float(v)
        if text == "0.2" and v < np.float32(0.2):
            found.setdefault("passes", sh)
        if text == "0.199999":
            found.setdefault("fails", sh)
    return cnt, edges([0, 2, 4, 6], [1, 3, 5, 7], [found["passes"], found["fails"], 0, 4])


def permuted(e, seed):
    p = np.random.default_rng(seed).permutation(len(e))
    return e[p], p
