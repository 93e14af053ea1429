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


HOSTILE = dict(stars=30, leaves=5, repeated=220, first_dropped=60, zero_count=24)


def hostile(seed, n_nodes, n_records):
    """(edges, k-mer counts, meta): a multigraph no writer of ours produces, seeded, every record at a random position.

      stars      30 disjoint stars of 5 leaves whose centres are joined in a ring: 30 nodes of degree 7 that no other record
                 names, ranked by id alone
      repeated   220 pairs 2 .. 6 times each, in both orientations, every copy with its own `shared`; at 0.20 some copies are
                 kept and some dropped in every column, and the lowest-index copy of the first 60 is dropped
      self       about 2 % of the records, kept and dropped
      outside    about 1 % of the records with one end >= n_nodes, on either side: n_nodes itself, 2^31, 0xFFFFFFFF, others
      zero       24 nodes counting 0 k-mers, each with a record that is infinite in avg and max, a NaN record and a record to
                 the next of them that is infinite in every column; the random records that name them add more
      rest       random ends among the nodes of no star, values around the threshold: test_derep_gpu._random_case

    meta: centres, repeated (the pairs (a, b), a < b), first_dropped (the first of them), zero, star_nodes, n_self, n_outside."""
    H = HOSTILE
    rng = np.random.default_rng([seed, n_nodes, n_records])
    perm = rng.permutation(n_nodes)
    n_star = H["stars"] * (H["leaves"] + 1)
    star_nodes, zero, plain = perm[:n_star], perm[n_star:n_star + H["zero_count"]], perm[n_star + H["zero_count"]:]
    assert len(plain) >= 2 * H["repeated"]
    cnt = rng.integers(3000, 4001, size=n_nodes).astype(np.uint32)
    cnt[zero] = 0
    centres, leaves = np.sort(star_nodes[:H["stars"]]), star_nodes[H["stars"]:].reshape(H["stars"], H["leaves"])
    s1, s2, frac, bump = [], [], [], []

    def add(a, b, f, k=0):
        s1.append(int(a)), s2.append(int(b)), frac.append(float(f)), bump.append(k)

    keep, drop = (lambda: rng.uniform(0.3, 0.45)), (lambda: rng.uniform(0.02, 0.15))   # kept / dropped in all three columns
    for c in range(H["stars"]):
        for leaf in leaves[c]:
            add(*((centres[c], leaf) if rng.random() < 0.5 else (leaf, centres[c])), keep())
        add(centres[c], centres[(c + 1) % H["stars"]], keep())
    pair_nodes = rng.choice(plain, size=(H["repeated"], 2), replace=False)        # (no node twice: the pairs are distinct)
    copies = []                                                                  # per pair: the logical indices of its copies
    for a, b in pair_nodes:
        k = int(rng.integers(2, 7))
        copies.append(list(range(len(s1), len(s1) + k)))
        for j in range(k):
            flip = j % 2 if j < 2 else rng.random() < 0.5                          # both orientations
            add(*((b, a) if flip else (a, b)), 0.0, j)
    n_self, n_out = max(2, n_records // 50), max(4, n_records // 100)
    for j in range(n_self):
        v = rng.choice(plain)
        add(v, v, keep() if j % 2 else drop())
    inside = np.concatenate([plain, zero])
    beyond = [0xFFFFFFFF, 0xFFFFFFFF, n_nodes, n_nodes, 1 << 31] + rng.integers(n_nodes, 1 << 32, size=n_out, dtype=np.uint64).tolist()
    first_out = len(s1)
    for j in range(n_out):
        v = rng.choice(inside)
        add(*((beyond[j], v) if j % 2 else (v, beyond[j])), keep())
    forced = {}                                                                  # logical index -> `shared`, whatever the counts
    for i, z in enumerate(zero):                                                 # inf in avg and max, NaN, inf in all three columns
        for a, b, sh in ((z, rng.choice(plain), int(rng.integers(1, 1500))), (rng.choice(plain), z, 0), (z, zero[(i + 1) % len(zero)], int(rng.integers(1, 1500)))):
            forced[len(s1)] = sh
            add(a, b, 0.0)
    n_fill = n_records - len(s1)
    assert n_fill > n_records // 4
    fa, fb = rng.choice(inside, size=n_fill), rng.choice(inside, size=n_fill)
    planted = {(min(int(x), int(y)), max(int(x), int(y))) for x, y in pair_nodes}
    for a, b, f in zip(fa, fb, rng.uniform(0.02, 0.4, size=n_fill)):
        if (min(int(a), int(b)), max(int(a), int(b))) in planted:                 # (no random copy of a planted pair)
            b = zero[0]
        add(a, b, f)
    pos = rng.permutation(n_records)                                             # logical record j stands at pos[j]
    frac = np.array(frac)
    for p, idx in enumerate(copies):                                             # kept / dropped by the order of the positions
        by_pos = sorted(idx, key=lambda j: pos[j])
        flags = ([False, True] if p < H["first_dropped"] else [True, False]) + [bool(rng.random() < 0.5) for _ in by_pos[2:]]
        for j, kept in zip(by_pos, flags):
            frac[j] = keep() if kept else drop()
    a, b = np.array(s1, dtype=np.uint64), np.array(s2, dtype=np.uint64)
    ca, cb = (np.where(x < n_nodes, cnt[np.minimum(x, n_nodes - 1).astype(np.int64)], 1).astype(np.float64) for x in (a, b))
    with np.errstate(divide="ignore"):
        shared = (frac * 2.0 / (1.0 / ca + 1.0 / cb)).astype(np.uint64) + np.array(bump, dtype=np.uint64)
    for idx in copies:                                                           # every copy its own `shared`
        seen = set()
        for j in idx:
            while int(shared[j]) in seen:
                shared[j] += 7
            seen.add(int(shared[j]))
    nil = (ca == 0) | (cb == 0)                                                 # an end of 0 k-mers: 0 shared (NaN, 0) or some (inf)
    shared[nil] = rng.integers(0, 1500, size=int(nil.sum())) * (rng.random(int(nil.sum())) < 0.7)
    shared[first_out:first_out + n_out] = KEEP
    for j, sh in forced.items():
        shared[j] = sh
    e = np.zeros(n_records, dtype=EDGE_DTYPE)
    e["source_1"][pos], e["source_2"][pos], e["shared"][pos] = a, b, shared
    meta = dict(centres=centres.tolist(), star_nodes=sorted(star_nodes.tolist()), zero=sorted(zero.tolist()), n_self=n_self, n_outside=n_out,
                repeated=[tuple(sorted((int(x), int(y)))) for x, y in pair_nodes])
    meta["first_dropped"] = meta["repeated"][:H["first_dropped"]]
    return e, cnt, meta


def via_after_permutation(e2, kept2, res, res2):
    """res over some records, res2 over the same records in the order e2 (kept2: its kept indices, ascending): rep, rank and
    degree are equal, and every member's via is the lowest kept index of e2 that names the member and its representative."""
    for k in ("rep", "rank", "degree"):
        assert (res[k] == res2[k]).all(), k
    first = {}
    s1, s2 = e2["source_1"].tolist(), e2["source_2"].tolist()
    for i in kept2:
        first.setdefault((min(s1[i], s2[i]), max(s1[i], s2[i])), int(i))
    rep = res["rep"].tolist()
    members = [v for v in range(len(rep)) if rep[v] != v]
    assert members
    for v in members:
        assert int(res2["via"][v]) == first[min(v, rep[v]), max(v, rep[v])], v
