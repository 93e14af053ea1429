"""Inputs of the cluster-report tests, built once for tests/test_report_cpu.py (which checks their stated properties without a GPU)
and tests/test_report_gpu.py.  The graph builders are those of tests/derep_inputs.py: ksp_edge records over sources of COUNT k-mers
each, so that shared / COUNT is exact and is the value of all three columns."""
import numpy as np

import derep_inputs as di
import repr_restate as rr

COUNT = di.COUNT
CHUNK = 2048                                   # (= engine.REPORT_CHUNK_EDGES; test_report_cpu.py checks it)
PATH_SIZES = [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
NAN = float("nan")


def path_case(n_edges):
    """(edges, counts, n_nodes): a path of n_edges records, ascending."""
    return di.path(n_edges + 1), di.same(n_edges + 1), n_edges + 1


def star_case(centre_first):
    """A star of 5 000 leaves: the centre is source_1 of every record (one run across waves and chunks) or source_2."""
    return di.star(5000, centre_first), di.same(5001), 5001


def clique_case():
    """A clique of 70 in ascending order: 2 415 records, more than one chunk, one label."""
    return di.clique(70), di.same(70), 70


def clique_and_paths(seed=5):
    """The clique's records shuffled, with ten disjoint paths of 8 records mixed in (their nodes behind the clique's).  Returns
    (edges, counts, n_nodes, the clique's records in their shuffled order)."""
    n_path, paths = di.disjoint_paths(80)
    paths["source_1"] += 70
    paths["source_2"] += 70
    both = np.concatenate([di.clique(70), paths])
    e, p = di.permuted(both, seed)
    return e, di.same(70 + n_path), 70 + n_path, e[p < 2415]


def hostile(seed=11, n_nodes=20000, n_records=2 * CHUNK + 1):
    """derep_inputs.hostile inside the report's domain: a record between two nodes whose value exceeds 1 in some column (shared above
    a count, or beside a count of 0) keeps its ends and loses its shared k-mers — it becomes a 0 or a NaN record, which every
    cut-off treats in its own way.  Self pairs, ends outside, repeated pairs in both orientations and NaN records stay."""
    e, cnt, meta = di.hostile(seed, n_nodes, n_records)
    inside = (e["source_1"] < n_nodes) & (e["source_2"] < n_nodes)
    over = np.zeros(len(e), dtype=bool)
    with np.errstate(invalid="ignore"):
        over[inside] = rr.column_values(e[inside], cnt, 5) > 1        # (the maximum: the other columns are not above it)
    e["shared"][over] = 0
    return e, cnt, meta


def orders(e):
    """The same records ascending by (source_1, source_2), reversed, and shuffled."""
    asc = e[np.lexsort((e["source_2"], e["source_1"]))]
    return {"ascending": asc, "reversed": asc[::-1].copy(), "shuffled": di.permuted(asc, 3)[0]}


# ---- graphs of at most 6 nodes with hand-written answers: (n_nodes, a, b, value, answer) --------------------------------------------
# answer: label, degree, strength / 2^30 (every value is a multiple of 0.25), via per node; per cluster (root, size, edges, nan_edges,
# sum_q / 2^30, min, max, medoid, covered)

SMALL = {
    # a path of 3: the middle node carries both records
    "path3": (3, [0, 1], [1, 2], [0.5, 0.5],
              dict(label=[0, 0, 0], degree=[1, 2, 1], strength=[2, 4, 2], via=[0, None, 1], cluster=[(0, 3, 2, 0, 4, 0.5, 0.5, 1, 2)])),
    # a clique of equal values: every strength is equal, the smallest node is the medoid
    "clique4": (4, [0, 0, 0, 1, 1, 2], [1, 2, 3, 2, 3, 3], [0.25] * 6,
                dict(label=[0] * 4, degree=[3] * 4, strength=[3] * 4, via=[None, 0, 1, 2], cluster=[(0, 4, 6, 0, 6, 0.25, 0.25, 0, 3)])),
    # two equal strengths: 1 and 2 both carry 0.75 + 0.5; the tie goes to node 1; node 3 hangs on 2 and is not covered
    "two_equal": (4, [0, 1, 2], [1, 2, 3], [0.5, 0.75, 0.5],
                  dict(label=[0] * 4, degree=[1, 2, 2, 1], strength=[2, 5, 5, 2], via=[0, None, 1, None], cluster=[(0, 4, 3, 0, 7, 0.5, 0.75, 1, 2)])),
    # a cluster of NaN records only beside a valued pair: no min, no max, no mean, the medoid is the smallest node
    "nan_only": (5, [0, 1, 3], [1, 2, 4], [NAN, NAN, 1.0],
                 dict(label=[0, 0, 0, 3, 3], degree=[1, 2, 1, 1, 1], strength=[0, 0, 0, 4, 4], via=[None, 0, None, None, 2],
                      cluster=[(0, 3, 2, 2, 0, NAN, NAN, 0, 1), (3, 2, 1, 0, 4, 1.0, 1.0, 3, 1)])),
    # a repeated pair, in both orientations: it counts again; via is the lowest index
    "repeated": (3, [0, 1, 0, 1], [1, 0, 1, 2], [0.25, 0.5, 0.25, 0.25],
                 dict(label=[0, 0, 0], degree=[3, 4, 1], strength=[4, 5, 1], via=[0, None, 3], cluster=[(0, 3, 4, 0, 5, 0.25, 0.5, 1, 2)])),
}


def small_records(name):
    """A SMALL graph as ksp_edge records whose value is the same in all three columns: sources of COUNT k-mers, except that both
    ends of a NaN record count 0 k-mers and share 0 (such a node carries NaN records alone in these graphs)."""
    n, a, b, v, _ = SMALL[name]
    cnt = di.same(n)
    shared = []
    for x, y, val in zip(a, b, v):
        if val != val:
            cnt[x] = cnt[y] = 0
            shared.append(0)
        else:
            shared.append(int(val * COUNT))
    return di.edges(a, b, shared), cnt, n


def specials():
    """(edges, counts, n_nodes, notes): NaN records (count 0, shared 0) of which one cluster holds nothing else, self pairs (valued,
    NaN and above 1: no part of anything), ends >= n_nodes, a repeated pair in both orientations, and records with shared = 0 beside
    positive counts (value 0: kept only at cut-off 0)."""
    n = 12
    cnt = di.same(n)
    cnt[[6, 7, 8]] = 0
    s1 = [0, 1, 0, 1, 2, 6, 7, 6, 3, 3, 8, 4, 12, 5, 0xFFFFFFFF, 9, 10, 4]
    s2 = [1, 0, 1, 2, 2, 7, 8, 6, 3, 4, 8, 12, 5, 1 << 31, 2, 10, 11, 5]
    sh = [di.KEEP, COUNT // 4, di.KEEP, COUNT, 2 * COUNT, 0, 0, 0, di.KEEP, di.KEEP, 5, di.KEEP, di.KEEP, di.KEEP, di.KEEP, 0, 0, COUNT // 8]
    notes = dict(nan_cluster=[6, 7, 8], zero_value=[15, 16], self_pairs=[4, 7, 8, 10], outside=[11, 12, 13, 14], repeated=[0, 1, 2])
    return di.edges(s1, s2, sh), cnt, n, notes


def boundary():
    """(edges, counts, cutoff): sources of 2^24 k-mers, so that shared / 2^24 is every float of [0.5, 1).  Record 0 has the value v
    whose printed text is the cut-off; record 1 the next float below, which prints a smaller text.  At that cut-off record 0 is kept
    and record 1 is not."""
    n = 1 << 24
    for s in range(int(0.7 * n), int(0.7 * n) - 200, -1):
        t1, t2 = "%.6g" % float(np.float32(s) / np.float32(n)), "%.6g" % float(np.float32(s - 1) / np.float32(n))
        if t1 != t2:
            return di.edges([0, 2], [1, 3], [s, s - 1]), np.full(4, n, dtype=np.uint32), float(t1)
    raise AssertionError("no boundary found")


def quantised():
    """(edges, counts): v = 2^-20 (shared 1 of 2^20: q = 2^12 exactly) and v = 1/3072 (q is truncated)."""
    cnt = np.array([COUNT, COUNT, 3072, 3072], dtype=np.uint32)
    return di.edges([0, 2], [1, 3], [1, 1]), cnt


def heavy(n_records=3_000_000):
    """One node of 3 * 10^6 records of value 1: its strength 3 * 10^6 * 2^32 is above 2^53, where doubles stop counting."""
    return di.edges(np.zeros(n_records, dtype=np.int64), np.ones(n_records, dtype=np.int64), COUNT), di.same(2), 2


def out_of_domain():
    """(edges, counts): a pair of value 0.5 and a pair whose shared k-mers exceed the count: 1.5."""
    return di.edges([0, 2], [1, 3], [di.KEEP, COUNT + COUNT // 2]), di.same(4)


# ---- k-mer counts that keep every value of a column at 6 significant digits or fewer -------------------------------------------------

def short_counts(n_sources, col, seed=7):
    """Counts from {16, 32, 64} for columns 3 / 5 (shared / a power of two up to 64 has at most 6 decimals), all 64 for column 4 (the
    average of two such values over different counts can need 7)."""
    if col == 4:
        return np.full(n_sources, 64, dtype=np.uint32)
    return np.random.default_rng(seed).choice(np.array([16, 32, 64], dtype=np.uint32), size=n_sources)


def short_index(col, n_sources=400, seed=7):
    """A colour index whose rows have at most 6 significant digits in column col: (color_off, sources as ids 1 .. n, colour weights,
    k-mer counts).  Groups of 1 .. 25 consecutive sources; a group shares one colour of weight 1 .. 6 and up to three colours of
    weight 1 .. 3 over random subsets, and its first source one colour of weight 1 with the first source of the next group: no pair
    shares more than 16 k-mers, the smallest count, so every value is k / 16, k / 32 or k / 64 and at most 1."""
    rng = np.random.default_rng([seed, col])
    counts = short_counts(n_sources, col, seed)
    colours, weights, first = [], [], []
    v = 0
    while v < n_sources:
        size = min(int(rng.integers(1, 26)), n_sources - v)
        group = np.arange(v, v + size)
        first.append(v)
        if size >= 2:
            colours.append(group)
            weights.append(int(rng.integers(1, 7)))
            for _ in range(int(rng.integers(0, 4))):
                colours.append(np.sort(rng.choice(group, size=int(rng.integers(2, size + 1)), replace=False)))
                weights.append(int(rng.integers(1, 4)))
        v += size
    for x, y in zip(first[::2], first[1::2]):                        # every other pair of neighbouring groups is joined
        colours.append(np.array([x, y]))
        weights.append(1)
    color_off = np.concatenate([[0], np.cumsum([len(c) for c in colours])]).astype(np.uint32)
    return color_off, (np.concatenate(colours) + 1).astype(np.uint32), np.array(weights, dtype=np.uint32), counts
