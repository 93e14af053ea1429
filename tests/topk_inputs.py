"""Seeded inputs of the top-k tests, built once for tests/test_topk_cpu.py (which checks without a GPU that they have the
properties the GPU tests rely on) and tests/test_topk_gpu.py.  The constants repeat KSP_TOPK_* of the header; the CPU test
compares them with kspider_amd.engine's."""
import numpy as np

import derep_inputs as di

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


def hubs(sizes, seed=0):
    """(edges, k-mer counts, n_nodes, hub nodes): hub i (node HUB_NODES[i]) has sizes[i] records, each to a leaf of its own, in a
    random orientation; SMALL nodes beside them with 2 x SMALL random records among themselves (a handful of entries each).  The
    leaves count one of three numbers of k-mers and a hub's records share 1 .. 6 k-mers, so a hub's values repeat many times
    over; max(12, n / 7) of its records share 7 with a leaf of 3 000 k-mers: the best value of the hub in every column, so that
    its first twelve places and more are ordered by the index alone.  Every record stands at a random position."""
    rng = np.random.default_rng([seed] + [int(s) for s in sizes])
    hub_nodes = list(HUB_NODES[:len(sizes)])
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
