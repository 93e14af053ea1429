"""Inputs of the query-mode tests (tests/test_query_gpu.py) and what they are expected to give.  A case is a pair of lists of
runs: the database's and the queries'.  The expectation is oracle.brute_pairs over the concatenation (database runs, then query
runs) filtered by the mode's rule; nothing here calls the code under test.  tests/test_query_inputs_cpu.py shows that every
builder makes the case it is named for."""
import numpy as np

import oracle
from kspider_amd import synth

CROSS, CROSS_AND_SELF = 0, 1
TOP = 2**64 - 1


def concat(db_runs, q_runs):
    """The sketch set of the concatenation: database sources 0 .. n_db - 1, then the queries."""
    return synth.from_runs(list(db_runs) + list(q_runs))


def split(sk, n_db):
    """(db_keys, db_offsets, q_keys, q_offsets) of a concatenated set whose first n_db sources are the database."""
    cut = int(sk.offsets[n_db])
    return sk.keys[:cut].copy(), sk.offsets[:n_db + 1].copy(), sk.keys[cut:].copy(), (sk.offsets[n_db:] - sk.offsets[n_db]).copy()


def filter_mode(edges, n_db, mode):
    """The rows of a table over the concatenation that the mode keeps: database x query, and in mode 1 also query x query."""
    keep = edges["source_2"] >= n_db
    if mode == CROSS:
        keep &= edges["source_1"] < n_db
    return edges[keep]


def expected(sk, n_db, mode):
    return filter_mode(oracle.brute_pairs(sk.keys, sk.offsets), n_db, mode)


def random_case(seed=4242, shuffle_seed=7, n_db=260):
    """smoke()'s generator, the runs shuffled so that the queries do not all fall into the last cluster."""
    sk = synth.generate("C2", n_sources=300, mean_size=400, cluster_cap=40, seed=seed)
    order = np.random.default_rng(shuffle_seed).permutation(sk.n_sources)
    runs = [sk.run(int(s)) for s in order]
    return runs[:n_db], runs[n_db:]


def one_bucket_case():
    """All 64 table keys share their high bits, so they sit in one bucket of the directory; the database holds keys of that
    bucket that are in the table, keys of it that are not (between table keys, and above the largest), and keys of other buckets."""
    base = 1 << 40
    q_runs = [[base + 16 * j + 2 * i for j in range(8)] for i in range(8)]   # even offsets 0 .. 126: 64 distinct keys
    db_runs = [[base + 1, base + 3, base + 77],                              # inside the bucket, odd: misses
               [base + 16, base + 18, base + 5, base + 2**36],               # two hits, a miss inside, a miss above the largest key
               [base - 1, 5, base + 126, base + 127]]                        # other buckets, the largest key, its neighbour
    return db_runs, q_runs


def hand_made_cases():
    """name -> (db_runs, q_runs)"""
    return {
        "empty_query": ([[1, 2], [3, 4]], [[], [1, 2, 3], []]),
        "empty_database_source": ([[], [1, 2], []], [[2, 3], [9]]),
        "query_equals_database_source": ([[5, 6, 7, 8], [1]], [[5, 6, 7, 8], [6]]),
        "one_hash_sources": ([[7], [8], [7]], [[7], [9], [8]]),
        "keys_0_and_top": ([[0, TOP], [0], [TOP], [5]], [[0, TOP], [TOP], [0, 7]]),
        "one_key_held_by_all": ([[42, 100 + i] for i in range(70)], [[42, 1000 + i] for i in range(20)]),
        "one_bucket": one_bucket_case(),
        "keys_outside_the_table": ([[1, 2, 3], [10**15, 10**15 + 1], [3, 500, 10**15]], [[500, 600], [600, 700, 800]]),
        "identical_queries": ([[2, 3, 4]], [[1, 2, 3], [1, 2, 3]]),
    }


def _universe_runs(rng, n, size, universe):
    return [rng.choice(universe, size=size, replace=False) for _ in range(n)]


def tile_case(n_q, seed=11):
    """n_q queries and 40 database sources of 30 hashes from 2 000 values: every tile of 64 queries has hits and misses."""
    rng = np.random.default_rng(seed + n_q)
    return _universe_runs(rng, 40, 30, 2000), _universe_runs(rng, n_q, 30, 2000)


LONG_RUN_LENGTHS = (255, 256, 257, 1000, 3, 40)


def long_run_case(seed=5):
    """Database runs of 255, 256, 257 and 1 000 entries (and two short ones) from 3 000 values, 12 queries of 200."""
    rng = np.random.default_rng(seed)
    return [rng.choice(3000, size=n, replace=False) for n in LONG_RUN_LENGTHS], _universe_runs(rng, 12, 200, 3000)


BLOCK_RUN_LENGTHS = (255, 256, 257, 1023, 1024, 1025, 3)
BLOCK_QUERY_LENGTH = 600


def block_case(seed=4):
    """Database runs one short of, exactly and one past what a wave (64 lanes x 4 keys = 256 entries) and a workgroup (1 024) look
    up in one step, and a run of 3, from 4 000 values; 6 queries of 600 from the same values.  (The seed: the run of 3 shares two
    keys with a query, so that gather at min_hashes 2 has it as a candidate.)"""
    rng = np.random.default_rng(seed)
    return [rng.choice(4000, size=n, replace=False) for n in BLOCK_RUN_LENGTHS], _universe_runs(rng, 6, BLOCK_QUERY_LENGTH, 4000)


def list_case(n_share):
    """Database source 0 shares the key 77 with n_share queries of two hashes each; source 1 shares it with none."""
    return [[77, 5], [6, 5]], [[77, 10**6 + i] for i in range(n_share)]


def expected_overflows(want, n_db, tile, capacity):
    """Emissions that cannot use the touched list: (probe source, query tile) pairs with more than `capacity` expected rows —
    a probe source touches exactly the queries it shares a key with."""
    if len(want) == 0:
        return 0
    q_tile = (want["source_2"].astype(np.int64) - n_db) // tile
    _, counts = np.unique(np.stack([want["source_1"].astype(np.int64), q_tile]), axis=1, return_counts=True)
    return int((counts > capacity).sum())
