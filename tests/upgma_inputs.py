"""Inputs of the UPGMA tests: every case is a function that returns (n_nodes, a, b, value) — two uint32 arrays of ends and the float32
values, one entry per record.  tests/test_upgma_cpu.py checks the properties the GPU tests rely on, without a GPU."""
import numpy as np

CHUNK = 2048                                                              # kspider_amd.engine.UPGMA_CHUNK_EDGES; asserted equal by the CPU test


def _case(n_nodes, a, b, value):
    return n_nodes, np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32), np.asarray(value, dtype=np.float32)


def sparse(n_nodes, n_records, seed, values=None):
    """A random sparse multigraph: ends uniform (self pairs and repeats happen), values k / 64 unless `values` lists them."""
    rng = np.random.default_rng([seed, n_nodes, n_records])
    a, b = rng.integers(0, n_nodes, n_records), rng.integers(0, n_nodes, n_records)
    v = rng.choice(values, n_records) if values is not None else rng.integers(1, 65, n_records) / 64.0
    return _case(n_nodes, a, b, v)


RECORD_COUNTS = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 17)


def path(n_nodes=300, equal=False):
    """0 - 1 - 2 - ...: strictly decreasing values (the bad case of the rounds), or one value (root order decides everything)."""
    i = np.arange(n_nodes - 1)
    return _case(n_nodes, i, i + 1, np.full(n_nodes - 1, 0.5) if equal else (60000 - 100 * i) / 65536.0)


def clique(n_nodes=40, value=0.75):
    a, b = np.triu_indices(n_nodes, 1)
    return _case(n_nodes, a, b, np.full(len(a), value))


def two_pairs_all_cross():
    """0-1 and 2-3 merge in round 1 while all four cross pairs exist: the fold of round 1 sums one run of exactly 4."""
    a = [0, 2, 0, 0, 1, 1]
    b = [1, 3, 2, 3, 2, 3]
    return _case(4, a, b, [0.9, 0.8, 0.1, 0.2, 0.3, 0.4])


def hub(leaves=5000, equal=False, seed=5):
    """Node 0 against `leaves` leaves: every pair offers to best[0]."""
    rng = np.random.default_rng(seed)
    v = np.full(leaves, 0.25) if equal else rng.permutation(leaves).astype(np.float64) / 8192.0 + 1.0 / 16384.0
    order = rng.permutation(leaves)
    return _case(leaves + 1, np.zeros(leaves)[order], (np.arange(leaves) + 1)[order], v[order])


def ignored_records():
    """(case, the records that take part): the pair 3-7 repeated 5 000 times beside self pairs, ends >= n_nodes, a NaN, a 0 and 2^-33."""
    n = 10
    a = [3] * 5000 + [1, 2, 12, 4, 5, 6, 8, 4000000000]
    b = [7] * 5000 + [1, 2, 3, 10, 6, 8, 9, 1]
    v = [0.125] * 5000 + [0.9, 1.0, 0.5, 0.5, float("nan"), 0.0, 2.0 ** -33, 0.5]
    return _case(n, a, b, v), 5000


def hostile_cross_product():
    """Two stars of 2 000 nodes (centres 0 and 2 000, every record 1.0) whose leaves are joined crosswise by 1 999 records of 2^-12, and
    the pair 4000-4001 repeated 5 000 times.  The stars complete first (a cross pair's similarity is at most 2^20 / 2^32, a star pair's
    at least 2^32 / 1999), so the last merge joins 2 000 x 2 000 nodes with S = 1999 * 2^20.  The repeated pair's S is chosen so that
    S * 4 000 000 = 2^64 + r with r < 2^22: against the last merge's S * 1 the two cross products differ only above bit 64."""
    target = -(-(1 << 56) // 15625)                                       # ceil(2^56 / 5^6): times 5^6 * 2^8 = 4 000 000 it is 2^64 + r
    q1 = (target // 5000) & ~0xFF                                         # 4 998 records of q1, one of q2, one of q3: floats all three
    rem = target - 4998 * q1
    q2 = rem & ~((1 << max(0, rem.bit_length() - 24)) - 1)
    q3 = rem - q2
    assert 0 < q1 < 1 << 32 and 0 < q2 <= 1 << 32 and 0 <= q3 < 256 and 4998 * q1 + q2 + q3 == target
    leaves = np.arange(1, 2000)
    a = np.concatenate([np.zeros(1999), np.full(1999, 2000), leaves, np.full(5000, 4000)])
    b = np.concatenate([leaves, 2000 + leaves, 2000 + leaves, np.full(5000, 4001)])
    v = np.concatenate([np.ones(1999), np.ones(1999), np.full(1999, 2.0 ** -12), np.array([q1] * 4998 + [q2, q3]) / 4294967296.0])
    rng = np.random.default_rng(8)
    order = rng.permutation(len(a))
    return _case(4002, a[order], b[order], v[order])


def orders(case):
    """The same records ascending, reversed, shuffled, and with source_1 > source_2."""
    n, a, b, v = case
    asc = np.lexsort((b, a))
    shuffled = np.random.default_rng(3).permutation(len(a))
    return {"ascending": (n, a[asc], b[asc], v[asc]), "reversed": (n, a[asc][::-1], b[asc][::-1], v[asc][::-1]),
            "shuffled": (n, a[shuffled], b[shuffled], v[shuffled]), "swapped": (n, np.maximum(a, b), np.minimum(a, b), v)}


def random_graph_2000():
    return sparse(2000, 6000, 11)


def tie_heavy_small(seed):
    """A multigraph of up to 14 nodes whose values come from a short list: heavy ties.  Values are q, not floats."""
    rng = np.random.default_rng([seed, 77])
    n = int(rng.integers(2, 15))
    m = int(rng.integers(0, 41))
    vals = [[1], [1, 2], [1, 2, 3, 6], list(range(1, 50))][int(rng.integers(0, 4))]
    return n, rng.integers(0, n, m), rng.integers(0, n, m), rng.choice(vals, m).astype(np.uint64)
