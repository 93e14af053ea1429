"""Seeded inputs of the top-k tests, built once for tests/test_topk_cpu.py (which checks without a GPU that they have the
properties the GPU tests rely on), tests/test_topk_gpu.py and tests/test_topk_paths_gpu.py.  The constants repeat KSP_TOPK_* of the header; the CPU test
compares them with kspider_amd.engine's."""
import numpy as np

import derep_inputs as di
import exact_values as xv

EDGE_DTYPE = di.EDGE_DTYPE
CHUNK = 2048
WAVE = 64            # entries up to which one wave selects
LDS = 4096           # entries up to which one workgroup selects in LDS; anything larger is streamed
MAX_K = 1024

CLASS_LIMIT_HUBS = (WAVE - 1, WAVE, WAVE + 1, LDS - 1, LDS, LDS + 1, 3 * LDS + 5)
SMALL = 300          # the nodes beside the hubs
HUB_NODES = (7, 120, 251)


def class_of(n: int) -> str:
    return "none" if n == 0 else "wave" if n <= WAVE else "workgroup" if n <= LDS else "stream"


def hubs(sizes, seed=0, hub_nodes=None):
    """(edges, k-mer counts, n_nodes, hub nodes): hub i (node HUB_NODES[i], or hub_nodes[i]) has sizes[i] records, each to a leaf of its own, in a
    random orientation; SMALL nodes beside them with 2 x SMALL random records among themselves (a handful of entries each).  The
    leaves count one of three numbers of k-mers and a hub's records share 1 .. 6 k-mers, so a hub's values repeat many times
    over; max(12, n / 7) of its records share 7 with a leaf of 3 000 k-mers: the best value of the hub in every column, so that
    its first twelve places and more are ordered by the index alone.  Every record stands at a random position."""
    rng = np.random.default_rng([seed] + [int(s) for s in sizes])
    hub_nodes = list(HUB_NODES[:len(sizes)] if hub_nodes is None else hub_nodes)
    assert len(hub_nodes) == len(sizes) and max(hub_nodes) < SMALL
    n_nodes = SMALL + int(sum(sizes))
    cnt = rng.integers(3000, 4001, size=n_nodes).astype(np.uint32)
    cnt[SMALL:] = rng.choice([3000, 3500, 4000], size=n_nodes - SMALL)
    s1, s2, sh = [], [], []
    leaf = SMALL
    for h, n in zip(hub_nodes, sizes):
        leaves = np.arange(leaf, leaf + n)
        leaf += n
        flip = rng.random(n) < 0.5
        s1.append(np.where(flip, leaves, h))
        s2.append(np.where(flip, h, leaves))
        sh.append(rng.integers(1, 7, size=n))
        top = rng.choice(n, size=max(12, n // 7), replace=False)
        sh[-1][top] = 7
        cnt[leaves[top]] = 3000
    plain = np.setdiff1d(np.arange(SMALL), hub_nodes)
    a, b = rng.choice(plain, size=2 * SMALL), rng.choice(plain, size=2 * SMALL)
    b = np.where(a == b, plain[(np.searchsorted(plain, a) + 1) % len(plain)], b)
    s1.append(a), s2.append(b), sh.append(rng.integers(1, 2000, size=2 * SMALL))
    e = di.edges(np.concatenate(s1), np.concatenate(s2), np.concatenate(sh))
    return e[rng.permutation(len(e))], cnt, n_nodes, hub_nodes


# one node per class for the k-against-the-segment cases: n entries, and the k values that stand around n where k may
SEGMENTS = (37, 200, LDS + 100)


def ks_around(n: int) -> list:
    """k = 1, n - 1, n, n + 1 where the segment is shorter than KSP_TOPK_MAX_K; a streamed segment is longer than every k, so
    there the two ends of the range stand in: 1 and KSP_TOPK_MAX_K."""
    return [1, n - 1, n, n + 1] if n + 1 <= MAX_K else [1, MAX_K]


TIES = ((40, 8), (500, 16), (LDS + 500, 100))     # (entries of the hub, k): one per class


def ties(n: int, k: int, seed=3):
    """hubs([n]) with k + 9 records of the hub raised to one and the same value above all others.  -> (edges, counts, n_nodes, hub,
    the positions of those records, ascending)."""
    e, cnt, n_nodes, (hub,) = hubs([n], seed)
    of_hub = np.nonzero((e["source_1"] == hub) | (e["source_2"] == hub))[0]
    best = np.sort(np.random.default_rng(seed).choice(of_hub, size=k + 9, replace=False))
    e["shared"][best] = 2999
    leaves = np.where(e["source_1"][best] == hub, e["source_2"][best], e["source_1"][best])
    cnt[leaves] = 3000
    return e, cnt, n_nodes, hub, best


def specials(seed=21, n_nodes=700, n_records=3 * CHUNK - 7):
    """derep_inputs.hostile — repeated pairs in both orientations, self pairs, ends >= n_nodes, sources of 0 k-mers with their NaN
    and +inf records, tied stars — and every twentieth record without shared k-mers (the value 0, or NaN beside a source of 0)."""
    e, cnt, meta = di.hostile(seed, n_nodes, n_records)
    e = e.copy()
    e["shared"][::20] = 0
    return e, cnt, meta


def orders(e, seed=5):
    """The same records ascending by (source_1, source_2), reversed, and at random positions."""
    asc = e[np.lexsort((e["source_2"], e["source_1"]))]
    return {"ascending": asc, "reversed": asc[::-1].copy(), "random": asc[np.random.default_rng(seed).permutation(len(e))]}


CHUNK_SIZES = (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 7)
N_RANDOM = 1500


def random_case(n: int, seed: int, n_nodes: int = N_RANDOM):
    rng = np.random.default_rng([seed, n])
    cnt = rng.choice([3000, 3500, 4000], size=n_nodes).astype(np.uint32)
    s1, s2 = rng.integers(0, n_nodes, size=n), rng.integers(0, n_nodes, size=n)
    shared = rng.integers(0, 60, size=n)              # few values: ties everywhere
    return di.edges(s1, s2, shared), cnt


def ranked_case(seed=9):
    """(n_nodes, a, b, rank): the ends of hubs([70, LDS + 50]) with ranks drawn from 12 numbers, 0 and 0xFFFFFFFF among them."""
    e, _, n_nodes, hub_nodes = hubs([70, LDS + 50], seed)
    rng = np.random.default_rng(seed)
    pool = np.array([0, 1, 2, 3, 5, 8, 1000, 1 << 20, 1 << 31, (1 << 31) + 1, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint64)
    return n_nodes, e["source_1"].copy(), e["source_2"].copy(), rng.choice(pool, size=len(e)).astype(np.uint32), hub_nodes


# ---- the inputs of tests/test_topk_paths_gpu.py: what the select kernels and the run-combining atomic do on lists built for them ----

RUN_LENGTHS = (1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 2047, 2048, 2049)
RUN_LAYOUTS = ("source_1", "source_2", "pair")
RUN_LEAD_IN = 37
RUN_GAP = 70
RUN_GAPS = {3: "self", 6: "outside", 9: "self", 11: "outside"}       # the stretch of non-entries behind run i
WAVE_RANGE = 512     # consecutive records of a chunk that one wave owns
# (run, kind, period, residue): the first record of that run, behind the run's first and behind the run's last such record, whose
# index is `residue` modulo `period` becomes a self pair or a record with an end >= n_nodes.  Lane = index % 64, so these are
# non-entries at lane 0 and at lane 63, at the first record of a wave's range and of a chunk, and at the last of both.
RUN_BREAKS = ((10, "self", 64, 0), (10, "outside", 64, 63), (11, "outside", WAVE_RANGE, WAVE_RANGE - 1), (11, "self", CHUNK, 0),
              (12, "self", 64, 17), (12, "outside", CHUNK, CHUNK - 1))


def sorted_runs(layout: str, lead_in: int = 0, seed=1):
    """(edges, k-mer counts, n_nodes, runs): run i, of RUN_LENGTHS[i] consecutive records, belongs to hub i (nodes 0 .. 13); each
    run starts where the last one ended, or behind the RUN_GAP non-entries of RUN_GAPS, and the whole list stands behind `lead_in`
    random records among nodes of their own.  layout "source_1": the hub is source_1 of every record of its run and source_2 a
    leaf of its own; "source_2": the other way round, a run in the second end while the first changes; "pair": one pair (hub i,
    node 14 + i) repeated for the whole run, a run in both ends at once.  All records of a run share the same number of k-mers
    with leaves of one size, so a run's order is the record index alone.  The self pairs of a gap name the hub before it and the
    outside records the hub behind it: the raw end continues the run, the entry does not.  RUN_BREAKS puts two non-entries into
    each of three runs.  runs: per run dict(hub, start, span, entries, broken: the indices of its non-entries)."""
    assert layout in RUN_LAYOUTS
    rng = np.random.default_rng([seed, lead_in])
    n_hubs = len(RUN_LENGTHS)
    n_lead = 12
    first_leaf = 2 * n_hubs + n_lead
    n_nodes = first_leaf + sum(RUN_LENGTHS)
    cnt = np.full(n_nodes, 4000, dtype=np.uint32)
    la = 2 * n_hubs + rng.integers(0, n_lead, size=lead_in)
    lb = 2 * n_hubs + (la - 2 * n_hubs + rng.integers(1, n_lead, size=lead_in)) % n_lead
    hub_end, other_end, shared, runs = [la], [lb], [rng.integers(1, 50, size=lead_in)], []
    at, leaf = lead_in, first_leaf
    for i, span in enumerate(RUN_LENGTHS):
        leaves = np.arange(leaf, leaf + span) if layout != "pair" else np.full(span, n_hubs + i)
        leaf += span
        cnt[leaves] = 3000 + 10 * i
        hubs_i = np.full(span, i)
        broken = []
        for run, kind, period, residue in RUN_BREAKS:
            if run != i:
                continue
            lo = broken[-1] + 1 if broken else at + 1
            p = lo + (residue - lo) % period
            assert p < at + span - 1, (i, kind, period, residue, at)
            leaves[p - at] = i if kind == "self" else n_nodes + 1
            broken.append(p)
        hub_end.append(hubs_i), other_end.append(leaves), shared.append(np.full(span, 100 + i))
        runs.append(dict(hub=i, start=at, span=span, entries=span - len(broken), broken=broken))
        at += span
        if i in RUN_GAPS:
            g = np.arange(RUN_GAP)
            hub_end.append(np.full(RUN_GAP, i) if RUN_GAPS[i] == "self" else np.full(RUN_GAP, i + 1))
            other_end.append(np.full(RUN_GAP, i) if RUN_GAPS[i] == "self" else n_nodes + g * 1000003)
            shared.append(np.full(RUN_GAP, 100 + i))
            at += RUN_GAP
    h, o = np.concatenate(hub_end), np.concatenate(other_end)
    e = di.edges(o, h, np.concatenate(shared)) if layout == "source_2" else di.edges(h, o, np.concatenate(shared))
    assert len(e) == at
    return e, cnt, n_nodes, runs


def sub_runs(e, n_nodes: int, end: str):
    """(node, start, stop) of every run of consecutive records that are entries of one and the same node in `end` ("source_1" or
    "source_2"): the runs for which the device makes one atomic per ballot."""
    s1, s2 = e["source_1"].astype(np.int64), e["source_2"].astype(np.int64)
    v = np.where((s1 < n_nodes) & (s2 < n_nodes) & (s1 != s2), e[end].astype(np.int64), -1)
    cut = np.nonzero(np.diff(v) != 0)[0] + 1
    start, stop = np.concatenate([[0], cut]), np.concatenate([cut, [len(v)]])
    keep = v[start] >= 0
    return v[start][keep], start[keep], stop[keep]


# adjacent nodes 0 .. 8: in the workgroup class every node is followed by one of another padded size (4 096, 128, 1 024, 256,
# 2 048, 128), and of the three streamed nodes the longest comes first
ADJACENT_HUBS = (LDS, 65, 1000, 129, 2048, 66, 2 * LDS + 7, LDS + 1, LDS + 300)


def adjacent_hubs():
    return hubs(ADJACENT_HUBS, seed=2, hub_nodes=range(len(ADJACENT_HUBS)))


REFILL_LAYOUTS = ("head_first", "rising", "equal", "few")
REFILL_LEAVES = 200
REFILL_KS = (1, 100, MAX_K)


def refill_case(layout: str, k: int, seed=4):
    """(n_nodes, a, b, rank, hub): LDS + 2 (LDS - k) + 1 ranked records that all name node 0 — four refills of LDS - k keys — and,
    in turn, one of REFILL_LEAVES other nodes (62 entries each at most: selected by a wave).
      head_first  the best k records stand among the first CHUNK and every later record is worse than all of them
      rising      the rank rises with the index: every refill replaces the whole head
      equal       one rank for all: the order is the index alone
      few         all ranks 0 except k - 1 records: the k-th place is a record of rank 0"""
    assert layout in REFILL_LAYOUTS and 1 <= k <= MAX_K
    rng = np.random.default_rng([seed, k])
    n = LDS + 2 * (LDS - k) + 1
    i = np.arange(n)
    leaf = 1 + i % REFILL_LEAVES
    flip = rng.random(n) < 0.5
    a, b = np.where(flip, leaf, 0), np.where(flip, 0, leaf)
    if layout == "head_first":
        rank = np.where(i < CHUNK, rng.integers(10, 21, size=n), rng.integers(0, 10, size=n))
        rank[rng.choice(CHUNK, size=k, replace=False)] += 100
    elif layout == "rising":
        rank = i + 1
    elif layout == "equal":
        rank = np.full(n, 7)
    else:
        rank = np.zeros(n, dtype=np.int64)
        rank[rng.choice(n, size=k - 1, replace=False)] = rng.integers(1, 4, size=k - 1)
    return 1 + REFILL_LEAVES, a.astype(np.uint32), b.astype(np.uint32), rank.astype(np.uint32), 0


SPECIAL_HUBS = (40, 500, LDS + 500)          # one per class
SPECIAL_KS = (30, 300, MAX_K)                # each above the entries of its hub that are numbers
SPECIAL_NUMBERS_MOST = 900                   # of the streamed hub: fewer than KSP_TOPK_MAX_K, so that k reaches its NaN entries
SPECIAL_ZERO_FIRST = 5                       # NaN records per hub with the source of 0 k-mers as source_1: 0, not NaN, in columns 3 and 5


def special_hubs(seed=6):
    """(edges, k-mer counts, n_nodes, hubs): nodes 0 .. 2 count 0 k-mers and have SPECIAL_HUBS records each, nodes 3 .. 5 have as
    many and count 3 500; every record goes to a leaf of its own, at a random position.  min(n / 3, SPECIAL_NUMBERS_MOST) records
    of a hub are numbers in every column and the others — two thirds of the two shorter hubs, four fifths of the streamed one,
    whose numbers must stay below KSP_TOPK_MAX_K — are NaN in column 4:
      hub of 0 k-mers    number: shared > 0, +inf in columns 4 and 5 beside shared / leaf in column 3; five of them to a leaf of 0
                         k-mers as well: +inf in every column.  NaN: shared = 0.
      hub of 3 500       number: half to a leaf of 0 k-mers with shared > 0 (+inf in 4 and 5), half to a leaf of 3 000 sharing 0 .. 6.
                         NaN: shared = 0 with a leaf of 0 k-mers.
    A NaN record names its source of 0 k-mers as source_2 — NaN in all three columns — except SPECIAL_ZERO_FIRST per hub."""
    rng = np.random.default_rng(seed)
    n_hubs = 2 * len(SPECIAL_HUBS)
    n_nodes = n_hubs + 2 * sum(SPECIAL_HUBS)
    cnt = np.full(n_nodes, 3000, dtype=np.uint32)
    cnt[:n_hubs] = [0, 0, 0, 3500, 3500, 3500]
    s1, s2, sh = [], [], []
    leaf = n_hubs
    for h in range(n_hubs):
        n = SPECIAL_HUBS[h % 3]
        numbers = min(n // 3, SPECIAL_NUMBERS_MOST)
        leaves = np.arange(leaf, leaf + n)
        leaf += n
        shared = np.zeros(n, dtype=np.int64)
        shared[:numbers] = rng.integers(1, 7, size=numbers)
        hub_first = rng.random(n) < 0.5
        if cnt[h] == 0:
            cnt[leaves[:5]] = 0
            hub_first[numbers:] = False                                   # the hub is the source of 0 k-mers: it stands second
            hub_first[numbers:numbers + SPECIAL_ZERO_FIRST] = True
        else:
            cnt[leaves[:numbers // 2]] = 0
            shared[numbers // 2:numbers] = rng.integers(0, 7, size=numbers - numbers // 2)
            cnt[leaves[numbers:]] = 0
            hub_first[numbers:] = True                                    # the leaf is the source of 0 k-mers
            hub_first[numbers:numbers + SPECIAL_ZERO_FIRST] = False
        s1.append(np.where(hub_first, h, leaves)), s2.append(np.where(hub_first, leaves, h)), sh.append(shared)
    e = di.edges(np.concatenate(s1), np.concatenate(s2), np.concatenate(sh))
    return e[rng.permutation(len(e))], cnt, n_nodes, list(range(n_hubs))


TILED_COPIES = (1, 8, 100)
# copies: (wave, workgroup, streamed) nodes of exact_values.hostile_edges(1) written `copies` times over
TILED_CLASSES = {1: (599, 0, 0), 8: (169, 430, 0), 100: (0, 592, 7)}
TILED_KS = {1: (49,), 8: (10, 400), 100: (10, MAX_K)}     # 49: the most entries of a node of one copy, so every entry is listed


def tiled(copies: int):
    """(edges, k-mer counts, n_nodes): the records of exact_values.hostile_edges(1) — counts and shared counts that are no exact
    floats, up to 2^64 - 1 — `copies` times one behind the other: a repeated pair is listed again and equal values fall back to
    the index."""
    h = xv.hostile_edges(1)
    return np.tile(h.edges, copies), h.kmer_counts, len(h.kmer_counts)


SMALL_NODES = (2, 63, 64, 65, 257)


def small_case(n_nodes: int, single: bool, seed=8):
    """(edges, k-mer counts): one record (0, n_nodes - 1), the only entry of the last node; or nine records, eight at random and that
    one behind them."""
    rng = np.random.default_rng([seed, n_nodes])
    cnt = rng.choice([3000, 3500, 4000], size=n_nodes).astype(np.uint32)
    if single:
        return di.edges([0], [n_nodes - 1], [5]), cnt
    n = 9
    a, b = rng.integers(0, n_nodes, size=n), rng.integers(0, n_nodes, size=n)
    a[-1], b[-1] = 0, n_nodes - 1
    return di.edges(a, b, rng.integers(0, 4, size=n)), cnt
